// Overlapping label groups: one sigmoid channel per group of label values (the KiTS / BraTS recipe of nnU-Net).
//   * the fused sigmoid + binary focal + Tversky loss over K group channels, forward sums, on-device finalize, backward;
//   * the sliding-window accumulate with an independent sigmoid per channel, and the merge that decodes the averaged
//     probabilities into a label map.
// The loss has the structure of loss.hip: one read of logits + labels per pass; per-thread fp32 partials -> wave shuffles
// -> LDS -> one double partial row per block -> fixed-order finalize (deterministic, no atomics, no host sync); row
// epilogue, row reduction, Tversky coefficients, pow_gamma and load_label are loss_core.h's.
//
// Definitions ("Label groups").  member[t], t in [0, T): bit k set iff label value t belongs to group k; the
// table travels by value in the launch arguments and the multi-hot target g_k(v) = bit k of member[t(v)] is never
// materialised.  Over the counted voxels (those not carrying the ignore label; M of them), p = sigmoid(z_k):
//   tp_k = sum p g, sp_k = sum p, sg_k = sum g
//   dice_k  = (tp_k + s) / (tp_k + alpha (sg_k - tp_k) + beta (sp_k - tp_k) + s)
//   focal_k = 1 / max(M, 1) sum_v [ (1-p)^gamma g softplus(-z) + p^gamma (1-g) softplus(z) ]
//   w       = weight_v / |weight_v|_1
//   Hybird  = sum_k w_k (1 - dice_k + focal_k); DiceLoss = sum w (1 - dice); Focal = sum w focal; Dice = sum w dice
// log p = -softplus(-z) and log(1 - p) = -softplus(z) come from the logit: sigmoid(40) == 1 in fp32, and the logarithm
// of a rounded 1 - p would be -inf.  A label outside [0, T) that is not the ignore label counts as a bad label (all
// channels off, loss NaN), reported through the state block like the softmax losses'.
#include "common.h"
#include "loss_core.h"

#define RU3D_GROUP_MAX_LABELS 32

// member[t] of the 32 label values, eight to a 64-bit word: read with three selects and a shift, so that the table
// stays in the scalar registers the launch arguments arrive in (a dynamically indexed byte array would go to scratch)
struct GroupTable {
    uint64_t word[RU3D_GROUP_MAX_LABELS / 8];
};
__device__ __forceinline__ int group_member(const GroupTable& tab, int t) {
    const uint64_t w = t < 16 ? (t < 8 ? tab.word[0] : tab.word[1]) : (t < 24 ? tab.word[2] : tab.word[3]);
    return (int)((w >> ((t & 7) * 8)) & 0xffu);
}

struct GroupState {
    RegionCoef r;    // first: bad_labels sits where every fused loss keeps it
    double counted;  // M
};

extern "C" size_t ru3d_group_loss_state_bytes(void) { return sizeof(GroupState); }

// a partial row: the REGION_Q quantities of the region losses (rows [blocks][REGION_Q], what region_reduce_rows reads),
// then the slot of the counted voxels (a second plane [blocks] behind the rows)
extern "C" size_t ru3d_group_loss_workspace_bytes(int n, int64_t v, int num_groups) {
    (void)num_groups;
    return (size_t)region_fwd_blocks((int64_t)n * v) * (REGION_Q + 1) * sizeof(double);
}

// what one channel of one voxel needs, from the logit: p = sigmoid(z), om = 1 - p (each rounded on its own, neither is
// 1 - the other), l = log(1 + exp(-|z|)), so that softplus(x) = max(x, 0) + l for x = z and x = -z
__device__ __forceinline__ void sigmoid_terms(float z, float& p, float& om, float& l) {
    const float e = expf(-fabsf(z));
    const float inv = 1.f / (1.f + e);
    const float lo = e * inv;
    l = log1pf(e);
    p = z >= 0.f ? inv : lo;
    om = z >= 0.f ? lo : inv;
}

// the label of voxel i -> its membership bits; false when the voxel carries the ignore label
__device__ __forceinline__ bool group_bits(const void* labels, int label_dtype, int64_t i, const GroupTable& tab,
                                           int num_labels, int has_ignore, int ignore_label, int& bits, int& bad) {
    const int t = load_label(labels, label_dtype, i);
    if (has_ignore && t == ignore_label) return false;
    if (t < 0 || t >= num_labels) {
        bad++;
        bits = 0;
    } else {
        bits = group_member(tab, t);
    }
    return true;
}

template <int K>
__global__ __launch_bounds__(256) void group_sums_kernel(const float* __restrict__ logits, int64_t stride_n,
                                                         int64_t stride_c, int64_t stride_v,
                                                         const void* __restrict__ labels, int label_dtype, int n,
                                                         int64_t v, float gamma, GroupTable tab, int num_labels,
                                                         int has_ignore, int ignore_label, double* __restrict__ part,
                                                         double* __restrict__ counted_part) {
    float tp[K], sp[K], sg[K], fo[K];
#pragma unroll
    for (int k = 0; k < K; k++) tp[k] = sp[k] = sg[k] = fo[k] = 0.f;
    int bad = 0, counted = 0;
    const int64_t total = (int64_t)n * v;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        int bits = 0;
        if (!group_bits(labels, label_dtype, i, tab, num_labels, has_ignore, ignore_label, bits, bad)) continue;
        counted++;
        const int64_t ni = i / v, vi = i - ni * v;
        const float* z = logits + ni * stride_n + vi * stride_v;
#pragma unroll
        for (int k = 0; k < K; k++) {
            const float zk = z[k * stride_c];
            float p, om, l;
            sigmoid_terms(zk, p, om, l);
            const bool g = (bits >> k) & 1;
            sp[k] += p;
            if (g) {
                tp[k] += p;
                sg[k] += 1.f;
                fo[k] += pow_gamma(om, gamma) * (fmaxf(-zk, 0.f) + l);
            } else {
                fo[k] += pow_gamma(p, gamma) * (fmaxf(zk, 0.f) + l);
            }
        }
    }
    region_write_row<K>(tp, sp, sg, fo, bad, part + (int64_t)blockIdx.x * REGION_Q);
    // a thread counts at most total / (2048 * 256) + 1 voxels: the wave sums are exact in fp32
    __shared__ float shc[4];
    const float wc = wave_sum((float)counted);
    if ((threadIdx.x & 63) == 0) shc[threadIdx.x >> 6] = wc;
    __syncthreads();
    if (threadIdx.x == 0) counted_part[blockIdx.x] = (double)shc[0] + (double)shc[1] + (double)shc[2] + (double)shc[3];
}

struct GroupParams {
    int kind, K;
    float alpha, beta, smooth;
    float w[RU3D_MAX_CLASSES];  // weight_v (un-normalised); all ones when the caller passed NULL
};

__global__ __launch_bounds__(REGION_LF_THREADS) void group_finalize_kernel(const double* __restrict__ part,
                                                                           const double* __restrict__ counted_part,
                                                                           int blocks, GroupParams P,
                                                                           GroupState* __restrict__ st,
                                                                           float* __restrict__ loss_out) {
    __shared__ double red[REGION_LF_GROUPS][REGION_Q];
    __shared__ double tot[REGION_Q];
    __shared__ double cred[REGION_LF_THREADS];
    region_reduce_rows(part, blocks, P.K, red, tot);
    // M: whole numbers, exact in any order; summed in a fixed one all the same
    double c = 0.0;
    for (int b = threadIdx.x; b < blocks; b += REGION_LF_THREADS) c += counted_part[b];
    cred[threadIdx.x] = c;
    __syncthreads();
    for (int s = REGION_LF_THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) cred[threadIdx.x] += cred[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    const double M = cred[0];
    // region_coefficients forms focal_k = C * fo_k / NV and its coefficient w_k * C / NV: with NV = K * max(M, 1) these
    // are fo_k / max(M, 1) and w_k / max(M, 1)
    const double NV = (double)P.K * (M < 1.0 ? 1.0 : M);
    loss_out[0] = (float)region_coefficients(P.kind, P.K, P.w, P.alpha, P.beta, P.smooth, NV, tot,
                                             (int)tot[4 * RU3D_MAX_CLASSES], &st->r);
    st->counted = M;
}

// d loss / d z_k of one voxel.  With s = -1, q = 1 - p for a member and s = +1, q = p otherwise, the focal term of the
// channel is q^gamma softplus(s z), and d/dz of it is s q^gamma (gamma (1 - q) softplus(s z) + q).
template <int K, typename TG>
__global__ __launch_bounds__(256) void group_bwd_kernel(const float* __restrict__ logits, int64_t stride_n,
                                                        int64_t stride_c, int64_t stride_v,
                                                        const void* __restrict__ labels, int label_dtype, int n,
                                                        int64_t v, float gamma, GroupTable tab, int num_labels,
                                                        int has_ignore, int ignore_label,
                                                        const GroupState* __restrict__ st,
                                                        const float* __restrict__ grad_out, TG* __restrict__ dz) {
    float qa[K], qb[K], qf[K];
#pragma unroll
    for (int k = 0; k < K; k++) {
        qa[k] = st->r.qa[k];
        qb[k] = st->r.qb[k];
        qf[k] = st->r.qf[k];
    }
    const float go = grad_out ? grad_out[0] : 1.f;
    const int64_t total = (int64_t)n * v;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t ni = i / v, vi = i - ni * v;
        const int64_t base = ni * stride_n + vi * stride_v;
        int bits = 0, bad = 0;
        if (!group_bits(labels, label_dtype, i, tab, num_labels, has_ignore, ignore_label, bits, bad)) {
#pragma unroll
            for (int k = 0; k < K; k++) dz[base + k * stride_c] = from_f32<TG>(0.f);
            continue;
        }
#pragma unroll
        for (int k = 0; k < K; k++) {
            const float zk = logits[base + k * stride_c];
            float p, om, l;
            sigmoid_terms(zk, p, om, l);
            const bool g = (bits >> k) & 1;
            const float q = g ? om : p, omq = g ? p : om;
            const float spl = fmaxf(g ? -zk : zk, 0.f) + l;
            const float df = pow_gamma(q, gamma) * (gamma * omq * spl + q);
            float d = p * om * (g ? qa[k] + qb[k] : qb[k]);  // dp/dz = p (1 - p)
            d += qf[k] * (g ? -df : df);
            dz[base + k * stride_c] = from_f32<TG>(d * go);
        }
    }
}

// num_groups has been checked (1 .. RU3D_MAX_CLASSES)
static int group_table_check(const char* who, int num_groups, const uint8_t* table, int num_labels, int has_ignore,
                             int ignore_label, GroupTable* out) {
    RU3D_REQUIRE(num_labels >= 1 && num_labels <= RU3D_GROUP_MAX_LABELS, "%s: %d label values unsupported (1..%d)", who,
                 num_labels, RU3D_GROUP_MAX_LABELS);
    RU3D_REQUIRE(table, "%s: null membership table", who);
    RU3D_REQUIRE(!has_ignore || ignore_label < 0 || ignore_label >= num_labels,
                 "%s: ignore label %d lies inside the label range [0, %d)", who, ignore_label, num_labels);
    for (int t = 0; t < RU3D_GROUP_MAX_LABELS / 8; t++) out->word[t] = 0;
    for (int t = 0; t < num_labels; t++) {
        RU3D_REQUIRE((table[t] >> num_groups) == 0, "%s: label value %d is a member of a group above %d", who, t,
                     num_groups - 1);
        out->word[t >> 3] |= (uint64_t)table[t] << ((t & 7) * 8);
    }
    return 0;
}

extern "C" int ru3d_group_loss_fwd(const float* logits, int64_t stride_n, int64_t stride_c, int64_t stride_v,
                                   const void* labels, int label_dtype, int n, int64_t v, int num_groups,
                                   const uint8_t* table, int num_labels, int has_ignore, int ignore_label, int kind,
                                   float gamma, const float* weight_v, float alpha, float beta, float smooth,
                                   void* state, float* loss_out, void* ws, size_t ws_bytes, void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    int rc = loss_view_check("group_loss_fwd", logits && labels && state && loss_out && ws, n > 0 && v > 0, label_dtype,
                             num_groups, 1, "groups");
    if (rc) return rc;
    GroupTable tab;
    rc = group_table_check("group_loss_fwd", num_groups, table, num_labels, has_ignore, ignore_label, &tab);
    if (rc) return rc;
    RU3D_REQUIRE(kind >= 0 && kind <= 3, "group_loss_fwd: bad kind %d", kind);
    RU3D_REQUIRE(ws_bytes >= ru3d_group_loss_workspace_bytes(n, v, num_groups), "group_loss_fwd: workspace too small");
    hipStream_t st = as_stream(stream);
    const int blocks = region_fwd_blocks((int64_t)n * v);
    double* part = (double*)ws;
    double* counted_part = part + (size_t)blocks * REGION_Q;
#define CALL(KK)                                                                                                     \
    hipLaunchKernelGGL(group_sums_kernel<KK>, dim3(blocks), dim3(256), 0, st, logits, stride_n, stride_c, stride_v, \
                       labels, label_dtype, n, v, gamma, tab, num_labels, has_ignore, ignore_label, part,           \
                       counted_part)
    RU3D_DISPATCH_C(1, num_groups, CALL)
#undef CALL
    rc = ru3d_check_launch("group_loss_sums");
    if (rc) return rc;
    GroupParams P;
    P.kind = kind;
    P.K = num_groups;
    P.alpha = alpha;
    P.beta = beta;
    P.smooth = smooth;
    fill_class_weights(P.w, weight_v, num_groups);
    hipLaunchKernelGGL(group_finalize_kernel, dim3(1), dim3(REGION_LF_THREADS), 0, st, (const double*)part,
                       (const double*)counted_part, blocks, P, (GroupState*)state, loss_out);
    return ru3d_check_launch("group_loss_finalize");
}

extern "C" int ru3d_group_loss_bwd(const float* logits, int64_t stride_n, int64_t stride_c, int64_t stride_v,
                                   const void* labels, int label_dtype, int n, int64_t v, int num_groups,
                                   const uint8_t* table, int num_labels, int has_ignore, int ignore_label, float gamma,
                                   const void* state, const float* grad_out, void* dlogits, int dlogits_dtype,
                                   void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    int rc = loss_view_check("group_loss_bwd", logits && labels && state && dlogits, n > 0 && v > 0, label_dtype,
                             num_groups, 1, "groups");
    if (rc) return rc;
    GroupTable tab;
    rc = group_table_check("group_loss_bwd", num_groups, table, num_labels, has_ignore, ignore_label, &tab);
    if (rc) return rc;
    RU3D_REQUIRE(dlogits_dtype == RU3D_F32 || dlogits_dtype == RU3D_BF16, "group_loss_bwd: bad dlogits dtype");
    hipStream_t st = as_stream(stream);
    const int blocks = flat_bwd_blocks((int64_t)n * v, 8192);
#define CALL(KK, TG)                                                                                                 \
    hipLaunchKernelGGL((group_bwd_kernel<KK, TG>), dim3(blocks), dim3(256), 0, st, logits, stride_n, stride_c, stride_v, \
                       labels, label_dtype, n, v, gamma, tab, num_labels, has_ignore, ignore_label,                 \
                       (const GroupState*)state, grad_out, (TG*)dlogits)
    RU3D_DISPATCH_C_DZ(1, num_groups, dlogits_dtype, CALL)
#undef CALL
    return ru3d_check_launch("group_loss_bwd");
}

// ------------------------------------------------------------------------------------------------ accumulate
// predict_accumulate_weighted_kernel (predict_tta.hip) with an independent sigmoid per channel in place of the softmax:
// one thread per window voxel, the logits read at the mirrored index, times (gx[a] * gy[j]) * gz[k], added into acc
// [X, Y, Z, K]; the weight added into cnt.  One thread owns a voxel of the window: no atomics, sums in launch order.
template <typename T, int K, bool WEIGHTED>
__global__ __launch_bounds__(256) void predict_accumulate_groups_kernel(
    const T* __restrict__ z, int ld, int pd, int ph, int pw, int flip, const float* __restrict__ gx,
    const float* __restrict__ gy, const float* __restrict__ gz, float* __restrict__ acc, float* __restrict__ cnt, int Y,
    int Z, int ox, int oy, int oz) {
    // no contraction: neither the weight nor a weighted probability is fused into the add that follows it, so cnt and acc
    // are sums of rounded fp32 products, numbers a host can form
#pragma clang fp contract(off)
    const int64_t total = (int64_t)pd * ph * pw;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int k = (int)(i % pw);
        const int64_t r = i / pw;
        const int j = (int)(r % ph);
        const int a = (int)(r / ph);
        const int sa = (flip & 1) ? pd - 1 - a : a;
        const int sj = (flip & 2) ? ph - 1 - j : j;
        const int sk = (flip & 4) ? pw - 1 - k : k;
        const T* zp = z + (((int64_t)sa * ph + sj) * pw + sk) * ld;
        float p[K];
#pragma unroll
        for (int c = 0; c < K; c++) p[c] = 1.f / (1.f + expf(-to_f32<T>(zp[c])));
        const int64_t o = ((int64_t)(ox + a) * Y + (oy + j)) * Z + (oz + k);
        float wgt = 1.f;
        if (WEIGHTED) {
            wgt = (gx[a] * gy[j]) * gz[k];
#pragma unroll
            for (int c = 0; c < K; c++) p[c] *= wgt;
        }
        float* ap = acc + o * K;
#pragma unroll
        for (int c = 0; c < K; c++) ap[c] += p[c];
        cnt[o] += wgt;
    }
}

template <int K>
static int accumulate_groups_launch(const ru3d_tensor* t, int dtype, int sample, int flip, const float* gx,
                                    const float* gy, const float* gz, float* acc, float* cnt, int Y, int Z, int ox,
                                    int oy, int oz, hipStream_t st) {
    const int64_t vox = (int64_t)t->d * t->h * t->w;
    const int64_t off = (int64_t)sample * vox * t->ld;
    int blocks = (int)((vox + 255) / 256);
    if (blocks > 2048) blocks = 2048;
#define RU3D_ACCG(T, WEIGHTED)                                                                                       \
    hipLaunchKernelGGL((predict_accumulate_groups_kernel<T, K, WEIGHTED>), dim3(blocks), dim3(256), 0, st,           \
                       (const T*)t->ptr + off, t->ld, t->d, t->h, t->w, flip, gx, gy, gz, acc, cnt, Y, Z, ox, oy, oz)
    if (dtype == RU3D_F32) {
        if (gx) RU3D_ACCG(float, true);
        else RU3D_ACCG(float, false);
    } else {
        if (gx) RU3D_ACCG(bf16, true);
        else RU3D_ACCG(bf16, false);
    }
#undef RU3D_ACCG
    return ru3d_check_launch("predict_accumulate_groups");
}

extern "C" int ru3d_predict_accumulate_groups(const ru3d_tensor* logits, int dtype, int sample, int flip,
                                              const float* gx, const float* gy, const float* gz, float* acc, float* cnt,
                                              int X, int Y, int Z, int ox, int oy, int oz, void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    RU3D_REQUIRE(tensor_ok(logits) && acc && cnt, "predict_accumulate_groups: bad argument");
    RU3D_REQUIRE(dtype == RU3D_F32 || dtype == RU3D_BF16, "predict_accumulate_groups: dtype must be f32 or bf16");
    RU3D_REQUIRE(sample >= 0 && sample < logits->n, "predict_accumulate_groups: sample %d outside batch of %d", sample,
                 logits->n);
    RU3D_REQUIRE(logits->c >= 1 && logits->c <= RU3D_MAX_CLASSES, "predict_accumulate_groups: %d groups (max %d)",
                 logits->c, RU3D_MAX_CLASSES);
    RU3D_REQUIRE(flip >= 0 && flip <= 7, "predict_accumulate_groups: mirror mask %d (0..7)", flip);
    RU3D_REQUIRE((gx && gy && gz) || (!gx && !gy && !gz),
                 "predict_accumulate_groups: the three weight tables come together or not at all");
    RU3D_REQUIRE(ox >= 0 && oy >= 0 && oz >= 0 && ox <= X - logits->d && oy <= Y - logits->h && oz <= Z - logits->w,
                 "predict_accumulate_groups: window [%d+%d, %d+%d, %d+%d] outside the %dx%dx%d volume", ox, logits->d,
                 oy, logits->h, oz, logits->w, X, Y, Z);
    hipStream_t st = as_stream(stream);
#define CALL(KK) \
    return accumulate_groups_launch<KK>(logits, dtype, sample, flip, gx, gy, gz, acc, cnt, Y, Z, ox, oy, oz, st)
    RU3D_DISPATCH_C(1, logits->c, CALL)
#undef CALL
    return 0;
}

// ------------------------------------------------------------------------------------------------ merge
// The decoding rule: channel k is on iff acc_k / cnt > threshold_k; the voxel's label is that of the LAST on channel in
// group order, 0 when none is on, when no window reached the voxel (cnt == 0) or when the mean is NaN.
struct GroupDecode {
    float threshold[RU3D_MAX_CLASSES];
    uint8_t label[RU3D_MAX_CLASSES];
};

template <int K>
__global__ __launch_bounds__(256) void predict_merge_groups_kernel(const float* __restrict__ acc,
                                                                   const float* __restrict__ cnt, int Y, int Z, int cx,
                                                                   int cy, int cz, int sx, int sy, int sz, GroupDecode D,
                                                                   uint8_t* __restrict__ out) {
    const int64_t total = (int64_t)sx * sy * sz;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int k = (int)(i % sz);
        const int64_t r = i / sz;
        const int j = (int)(r % sy);
        const int a = (int)(r / sy);
        const int64_t o = ((int64_t)(cx + a) * Y + (cy + j)) * Z + (cz + k);
        const float n = cnt[o];
        uint8_t label = 0;
        if (n != 0.f) {
#pragma unroll
            for (int c = 0; c < K; c++)
                if (acc[o * K + c] / n > D.threshold[c]) label = D.label[c];  // a NaN mean compares false
        }
        out[i] = label;
    }
}

extern "C" int ru3d_predict_merge_groups(const float* acc, const float* cnt, int X, int Y, int Z, int num_groups,
                                         const int32_t* group_labels, const float* threshold, int cx, int cy, int cz,
                                         int sx, int sy, int sz, uint8_t* out, void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    RU3D_REQUIRE(acc && cnt && out && group_labels && threshold, "predict_merge_groups: bad argument");
    RU3D_REQUIRE(num_groups >= 1 && num_groups <= RU3D_MAX_CLASSES, "predict_merge_groups: %d groups (max %d)",
                 num_groups, RU3D_MAX_CLASSES);
    RU3D_REQUIRE(sx > 0 && sy > 0 && sz > 0 && cx >= 0 && cy >= 0 && cz >= 0 && cx <= X - sx && cy <= Y - sy &&
                     cz <= Z - sz,
                 "predict_merge_groups: crop [%d+%d, %d+%d, %d+%d] outside the %dx%dx%d volume", cx, sx, cy, sy, cz, sz,
                 X, Y, Z);
    GroupDecode D;
    for (int k = 0; k < RU3D_MAX_CLASSES; k++) {
        D.threshold[k] = 0.f;
        D.label[k] = 0;
        if (k >= num_groups) continue;
        RU3D_REQUIRE(group_labels[k] >= 0 && group_labels[k] <= 255, "predict_merge_groups: label %d of group %d (0..255)",
                     group_labels[k], k);
        RU3D_REQUIRE(threshold[k] == threshold[k], "predict_merge_groups: threshold of group %d is NaN", k);
        D.threshold[k] = threshold[k];
        D.label[k] = (uint8_t)group_labels[k];
    }
    hipStream_t st = as_stream(stream);
    const int64_t vox = (int64_t)sx * sy * sz;
    int blocks = (int)((vox + 255) / 256);
    if (blocks > 8192) blocks = 8192;
#define CALL(KK)                                                                                                     \
    hipLaunchKernelGGL((predict_merge_groups_kernel<KK>), dim3(blocks), dim3(256), 0, st, acc, cnt, Y, Z, cx, cy, cz, \
                       sx, sy, sz, D, out)
    RU3D_DISPATCH_C(1, num_groups, CALL)
#undef CALL
    return ru3d_check_launch("predict_merge_groups");
}
