// Deep supervision: the fused softmax + focal + Tversky loss of loss.hip on EVERY supervised decoder level at once - one
// sums launch and one finalize for all levels, one backward launch for all levels - against ONE full-resolution label
// tensor.  Level l (shift s) never gets labels of its own: voxel (a, b, c) of that level reads label[a << s][b << s][c << s]
// (label[:, ::2**s, ::2**s, ::2**s]: nearest-neighbour down-sampling with the integer step 2**s).
//
// Same arithmetic and precisions as loss_sums_kernel / loss_finalize_kernel / loss_bwd_kernel, level by level: float32 per
// voxel, per-thread float32 partials -> wave shuffles -> LDS -> one float64 partial row per block -> a fixed-order finalize
// by one workgroup (deterministic, no atomics, no host sync).  A block belongs to one level: the kernels' grid is the
// concatenation of the levels' block ranges, and the level table with the ranges rides in the kernel arguments (the block
// map of adam_multi_kernel with 8 entries: a block finds its level by comparing its index with at most 8 range starts).
//   total = sum_l w_l * loss_l,  dlogits_l = w_l * grad_out * d loss_l / d logits_l
// w_l is read from device memory by the finalize (block[0 .. 7]) and parked in the state block for the backward, so a
// captured step follows a rewritten weight without a recapture and a backward uses the weights of its own forward.
//
// Traffic: level 0 reads C planes (NCDHW) or C-wide rows (NDHWC) at unit stride plus one label per voxel.  A level at
// shift s >= 1 touches every 2**s-th label of every 2**s-th row - a strided read that wastes most of each line - but all
// aux levels together hold at most 1/7 of level 0's voxels, so it is left as it is.
#include "common.h"
#include <stddef.h>

#define RU3D_MAX_CLASSES 8

// per level: the layout of loss.hip's LossState (sums, backward coefficients, loss, bad label count), so that level 0's
// count of out-of-range labels sits where every fused loss keeps it
struct DsLevelState {
    double sums[4][RU3D_MAX_CLASSES];  // tp, sp, sg, foc
    float qa[RU3D_MAX_CLASSES];        // dL/dp_c = qa_c * g_c + qb_c  (+ focal term)
    float qb[RU3D_MAX_CLASSES];
    float qf[RU3D_MAX_CLASSES];
    float loss;
    int bad_labels;                    // level 0 only
    float weight;                      // w_l of this forward
    int pad;
};

struct DsState {
    DsLevelState lev[RU3D_DS_MAX_LEVELS];
    float total;
    int levels;
    int pad[2];
};

struct DsLevelArg {
    const float* logits;
    float* dlogits;
    int64_t stride_n, stride_c, stride_v;
    int64_t v;      // d * h * w
    int h, w, shift, block0;      // block0: first block of the level's range; its length is block0 of the next level
};

struct DsArgs {
    DsLevelArg lev[RU3D_DS_MAX_LEVELS];
    int levels, nblocks;      // nblocks: end of the last range
    int n, label_dtype;
    int D, H, W, pad;
    const void* labels;
};

struct DsParams {
    int kind, C, levels;
    float gamma, alpha, beta, smooth;
    float w[RU3D_MAX_CLASSES];  // weight_v (un-normalised); all ones when the caller passed NULL
    int blocks[RU3D_DS_MAX_LEVELS + 1];
    double nv[RU3D_DS_MAX_LEVELS];
};

__device__ __forceinline__ int ds_load_label(const void* labels, int label_dtype, int64_t i) {
    if (label_dtype == RU3D_LABEL_I64) return (int)((const int64_t*)labels)[i];
    return (int)((const uint8_t*)labels)[i];
}

__device__ __forceinline__ float ds_pow_gamma(float base, float gamma) {
    if (gamma == 2.f) return base * base;
    if (gamma == 1.f) return base;
    if (gamma == 0.f) return 1.f;
    return powf(base, gamma);
}

// probabilities + log-probabilities of one voxel (softmax over C, sigmoid for C == 1): loss.hip's voxel_probs
template <int C>
__device__ __forceinline__ void ds_voxel_probs(const float* __restrict__ z, int64_t stride_c, float (&p)[C], float (&lp)[C]) {
    float zz[C];
#pragma unroll
    for (int c = 0; c < C; c++) zz[c] = z[c * stride_c];
    if (C == 1) {
        const float pr = 1.f / (1.f + __expf(-zz[0]));
        p[0] = pr;
        lp[0] = logf(pr);
        return;
    }
    float m = zz[0];
#pragma unroll
    for (int c = 1; c < C; c++) m = fmaxf(m, zz[c]);
    float se = 0.f;
#pragma unroll
    for (int c = 0; c < C; c++) se += expf(zz[c] - m);
    const float lse = logf(se);
#pragma unroll
    for (int c = 0; c < C; c++) {
        lp[c] = zz[c] - m - lse;
        p[c] = expf(lp[c]);
    }
}

// the level a block works on (ranges are consecutive and not empty)
__device__ __forceinline__ int ds_level_of(const DsArgs& A, int block) {
    int l = 0;
#pragma unroll
    for (int k = 1; k < RU3D_DS_MAX_LEVELS; k++)
        if (k < A.levels && block >= A.lev[k].block0) l = k;
    return l;
}

// index of the full-resolution label that voxel vi of sample ni of a level picks
__device__ __forceinline__ int64_t ds_label_index(const DsArgs& A, const DsLevelArg& Lv, int64_t ni, int64_t vi) {
    if (Lv.shift == 0) return ni * Lv.v + vi;      // level 0 has the labels' extents
    const int64_t row = vi / Lv.w;
    const int c = (int)(vi - row * Lv.w);
    const int64_t a = row / Lv.h;
    const int b = (int)(row - a * Lv.h);
    return ((ni * A.D + (a << Lv.shift)) * A.H + ((int64_t)b << Lv.shift)) * A.W + ((int64_t)c << Lv.shift);
}

template <int C>
__global__ __launch_bounds__(256) void ds_sums_kernel(DsArgs A, float gamma, double* __restrict__ part) {
    const int l = ds_level_of(A, blockIdx.x);
    const DsLevelArg Lv = A.lev[l];
    const int first = Lv.block0;
    const int count = ((l + 1 < A.levels) ? A.lev[l + 1].block0 : A.nblocks) - first;
    float tp[C], sp[C], sg[C], fo[C];
#pragma unroll
    for (int c = 0; c < C; c++) tp[c] = sp[c] = sg[c] = fo[c] = 0.f;
    int bad = 0;
    const int64_t total = (int64_t)A.n * Lv.v;
    for (int64_t i = (int64_t)(blockIdx.x - first) * 256 + threadIdx.x; i < total; i += (int64_t)count * 256) {
        const int64_t ni = i / Lv.v, vi = i - ni * Lv.v;
        float p[C], lp[C];
        ds_voxel_probs<C>(Lv.logits + ni * Lv.stride_n + vi * Lv.stride_v, Lv.stride_c, p, lp);
        int t = ds_load_label(A.labels, A.label_dtype, ds_label_index(A, Lv, ni, vi));
        if (t < 0 || t >= C) {
            bad++;
            t = -1;
        }
#pragma unroll
        for (int c = 0; c < C; c++) {
            sp[c] += p[c];
            if (c == t) {
                tp[c] += p[c];
                sg[c] += 1.f;
                fo[c] += -ds_pow_gamma(1.f - p[c], gamma) * lp[c];
            }
        }
    }
    __shared__ double sh[4][4 * C + 1];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < C; c++) {
        const float a = wave_sum(tp[c]), b = wave_sum(sp[c]), d = wave_sum(sg[c]), e = wave_sum(fo[c]);
        if (lane == 0) {
            sh[wid][0 * C + c] = a;
            sh[wid][1 * C + c] = b;
            sh[wid][2 * C + c] = d;
            sh[wid][3 * C + c] = e;
        }
    }
    const float fb = wave_sum((float)bad);
    if (lane == 0) sh[wid][4 * C] = fb;
    __syncthreads();
    if (threadIdx.x < 4 * C + 1) {
        const int q = threadIdx.x;
        const double s = sh[0][q] + sh[1][q] + sh[2][q] + sh[3][q];
        // partial layout: [block][4*MAX + 1]
        const int dst = (q == 4 * C) ? 4 * RU3D_MAX_CLASSES : (q / C) * RU3D_MAX_CLASSES + (q % C);
        part[(int64_t)blockIdx.x * (4 * RU3D_MAX_CLASSES + 1) + dst] = s;
    }
}

// One workgroup of 1024 threads, level after level: loss_finalize_kernel's reduction of the level's partial rows (thread
// (g, q) sums quantity q over the rows g, g + NG, ..., then the NG group sums are added in group order), thread 0 turns the
// sums into the level's loss and backward coefficients.  block: float32 [0 .. 7] the level weights (read),
// [8 .. 15] the levels' losses and [16] the total (written).
constexpr int DS_LF_THREADS = 1024;
__global__ __launch_bounds__(DS_LF_THREADS) void ds_finalize_kernel(const double* __restrict__ part, DsParams P,
                                                                    float* __restrict__ block, DsState* __restrict__ st,
                                                                    float* __restrict__ loss_out) {
    constexpr int Q = 4 * RU3D_MAX_CLASSES + 1;
    constexpr int NG = DS_LF_THREADS / Q;
    __shared__ double red[NG][Q];
    __shared__ double tot[Q];
    double total = 0.0;      // thread 0's
    for (int l = 0; l < P.levels; l++) {
        const double* pl = part + (int64_t)P.blocks[l] * Q;
        const int blocks = P.blocks[l + 1] - P.blocks[l];
        const int g = threadIdx.x / Q, q = threadIdx.x % Q;
        if (g < NG) {
            double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
            int b = g;
            for (; b + 3 * NG < blocks; b += 4 * NG) {
                s0 += pl[(int64_t)b * Q + q];
                s1 += pl[(int64_t)(b + NG) * Q + q];
                s2 += pl[(int64_t)(b + 2 * NG) * Q + q];
                s3 += pl[(int64_t)(b + 3 * NG) * Q + q];
            }
            for (; b < blocks; b += NG) s0 += pl[(int64_t)b * Q + q];
            red[g][q] = (s0 + s1) + (s2 + s3);
        }
        __syncthreads();
        if (threadIdx.x < Q) {
            const int qq = threadIdx.x, c = qq % RU3D_MAX_CLASSES;
            double t = 0.0;
            if (!(qq < 4 * RU3D_MAX_CLASSES && c >= P.C))
                for (int k = 0; k < NG; k++) t += red[k][qq];
            tot[qq] = t;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            DsLevelState* sl = &st->lev[l];
            const int C = P.C;
            double wsum = 0.0;
            for (int c = 0; c < C; c++) wsum += fabs((double)P.w[c]);
            if (wsum < 1e-12) wsum = 1e-12;  // F.normalize eps
            const double NV = P.nv[l];
            const bool has_dice = P.kind != RU3D_LOSS_FOCAL;
            const bool has_focal = (P.kind == RU3D_LOSS_HYBIRD) || (P.kind == RU3D_LOSS_FOCAL);
            double loss = 0.0;
            for (int c = 0; c < RU3D_MAX_CLASSES; c++) {
                sl->qa[c] = sl->qb[c] = sl->qf[c] = 0.f;
                for (int k = 0; k < 4; k++) sl->sums[k][c] = tot[k * RU3D_MAX_CLASSES + c];
            }
            for (int c = 0; c < C; c++) {
                const double w = (double)P.w[c] / wsum;
                const double tp = tot[0 * RU3D_MAX_CLASSES + c], sp = tot[1 * RU3D_MAX_CLASSES + c],
                             sg = tot[2 * RU3D_MAX_CLASSES + c], fo = tot[3 * RU3D_MAX_CLASSES + c];
                double term = 0.0;
                if (has_dice) {
                    const double a = P.alpha, b = P.beta, s = P.smooth;
                    const double den = tp + a * (sg - tp) + b * (sp - tp) + s;
                    const double dice = (tp + s) / den;
                    term += 1.0 - dice;
                    // d dice / d p_c(v) = g * A - B
                    const double A = (den - (tp + s) * (1.0 - a - b)) / (den * den);
                    const double B = (tp + s) * b / (den * den);
                    sl->qa[c] = (float)(-w * A);
                    sl->qb[c] = (float)(w * B);
                }
                if (has_focal) {
                    term += (double)C * fo / NV;
                    sl->qf[c] = (float)(w * (double)C / NV);
                }
                loss += w * term;
            }
            // out-of-range labels are counted where every label is read once: on level 0
            sl->bad_labels = (l == 0) ? (int)tot[4 * RU3D_MAX_CLASSES] : 0;
            if (sl->bad_labels > 0) loss = nan("");  // F.one_hot would have raised (loss.py:27)
            const float wl = block[l];
            sl->weight = wl;
            sl->loss = (float)loss;
            sl->pad = 0;
            block[RU3D_DS_MAX_LEVELS + l] = (float)loss;
            total += (double)wl * loss;
        }
        __syncthreads();      // red / tot are rewritten by the next level
    }
    if (threadIdx.x != 0) return;
    st->total = (float)total;
    st->levels = P.levels;
    block[2 * RU3D_DS_MAX_LEVELS] = (float)total;
    loss_out[0] = (float)total;
}

template <int C>
__global__ __launch_bounds__(256) void ds_bwd_kernel(DsArgs A, float gamma, const DsState* __restrict__ st,
                                                     const float* __restrict__ grad_out) {
    const int l = ds_level_of(A, blockIdx.x);
    const DsLevelArg Lv = A.lev[l];
    const int first = Lv.block0;
    const int count = ((l + 1 < A.levels) ? A.lev[l + 1].block0 : A.nblocks) - first;
    const DsLevelState* sl = &st->lev[l];
    float qa[C], qb[C], qf[C];
#pragma unroll
    for (int c = 0; c < C; c++) {
        qa[c] = sl->qa[c];
        qb[c] = sl->qb[c];
        qf[c] = sl->qf[c];
    }
    const float go = (grad_out ? grad_out[0] : 1.f) * sl->weight;
    const int64_t total = (int64_t)A.n * Lv.v;
    for (int64_t i = (int64_t)(blockIdx.x - first) * 256 + threadIdx.x; i < total; i += (int64_t)count * 256) {
        const int64_t ni = i / Lv.v, vi = i - ni * Lv.v;
        const int64_t base = ni * Lv.stride_n + vi * Lv.stride_v;
        float p[C], lp[C], u[C];
        ds_voxel_probs<C>(Lv.logits + base, Lv.stride_c, p, lp);
        const int t = ds_load_label(A.labels, A.label_dtype, ds_label_index(A, Lv, ni, vi));
        float su = 0.f;
#pragma unroll
        for (int c = 0; c < C; c++) {
            // u_c = p_c * dL/dp_c, written so that p -> 0 stays finite
            float uc = p[c] * qb[c];
            if (c == t) {
                const float om = 1.f - p[c];
                uc += p[c] * qa[c];
                float dfp;  // p * d/dp[ -(1-p)^g log p ] = g (1-p)^(g-1) p log p - (1-p)^g
                if (gamma == 2.f)
                    dfp = 2.f * om * p[c] * lp[c] - om * om;
                else if (gamma == 0.f)
                    dfp = -1.f;
                else
                    dfp = gamma * powf(om, gamma - 1.f) * p[c] * lp[c] - powf(om, gamma);
                uc += qf[c] * dfp;
            }
            u[c] = uc;
            su += uc;
        }
#pragma unroll
        for (int c = 0; c < C; c++) {
            float d;
            if (C == 1)
                d = u[0] * (1.f - p[0]);  // sigmoid: dp/dz = p (1 - p)
            else
                d = u[c] - p[c] * su;
            Lv.dlogits[base + c * Lv.stride_c] = d * go;
        }
    }
}

// the levels' block ranges: ceil(n v_l / per_block) blocks each, at most `cap` (a block then strides over its level)
static int ds_fill_args(DsArgs& A, const ru3d_ds_level* levels, void* const* dlogits, int num_levels, const void* labels,
                 int label_dtype, int n, int D, int H, int W, int per_block, int cap, const char* what) {
    RU3D_REQUIRE(levels && labels, "%s: null pointer", what);
    RU3D_REQUIRE(num_levels >= 1 && num_levels <= RU3D_DS_MAX_LEVELS, "%s: %d levels (1 .. %d)", what, num_levels,
                 RU3D_DS_MAX_LEVELS);
    RU3D_REQUIRE(n > 0 && D > 0 && H > 0 && W > 0, "%s: empty input", what);
    RU3D_REQUIRE(label_dtype == RU3D_LABEL_I64 || label_dtype == RU3D_LABEL_U8, "%s: bad label dtype", what);
    A.levels = num_levels;
    A.n = n;
    A.label_dtype = label_dtype;
    A.D = D;
    A.H = H;
    A.W = W;
    A.pad = 0;
    A.labels = labels;
    int64_t next = 0;
    for (int l = 0; l < RU3D_DS_MAX_LEVELS; l++) {
        DsLevelArg& Lv = A.lev[l];
        if (l >= num_levels) {
            Lv = DsLevelArg{};
            continue;
        }
        const ru3d_ds_level& in = levels[l];
        RU3D_REQUIRE(in.logits, "%s: level %d has no logits", what, l);
        RU3D_REQUIRE(in.d > 0 && in.h > 0 && in.w > 0 && in.shift >= 0 && in.shift <= 24, "%s: level %d: bad extents or shift",
                     what, l);
        // every label a level picks lies inside the label tensor
        RU3D_REQUIRE(((int64_t)(in.d - 1) << in.shift) <= D - 1 && ((int64_t)(in.h - 1) << in.shift) <= H - 1 &&
                         ((int64_t)(in.w - 1) << in.shift) <= W - 1,
                     "%s: level %d (%d x %d x %d at shift %d) reaches outside the %d x %d x %d labels", what, l, in.d, in.h,
                     in.w, in.shift, D, H, W);
        if (l == 0)
            RU3D_REQUIRE(in.shift == 0 && in.d == D && in.h == H && in.w == W,
                         "%s: level 0 must have the labels' extents (shift 0)", what);
        Lv.logits = in.logits;
        Lv.dlogits = dlogits ? (float*)dlogits[l] : nullptr;
        RU3D_REQUIRE(!dlogits || Lv.dlogits, "%s: level %d has no dlogits", what, l);
        Lv.stride_n = in.stride_n;
        Lv.stride_c = in.stride_c;
        Lv.stride_v = in.stride_v;
        Lv.v = (int64_t)in.d * in.h * in.w;
        Lv.h = in.h;
        Lv.w = in.w;
        Lv.shift = in.shift;
        Lv.block0 = (int)next;
        int64_t b = ((int64_t)n * Lv.v + per_block - 1) / per_block;
        if (b > cap) b = cap;
        if (b < 1) b = 1;
        next += b;
    }
    A.nblocks = (int)next;
    return 0;
}

constexpr int DS_FWD_PER_BLOCK = 256 * 8, DS_FWD_CAP = 2048;      // loss_blocks() of loss.hip, per level
constexpr int DS_BWD_PER_BLOCK = 256 * 2, DS_BWD_CAP = 8192;

static int ds_fwd_blocks(const ru3d_ds_level* levels, int num_levels, int n) {
    int64_t total = 0;
    for (int l = 0; l < num_levels; l++) {
        int64_t b = ((int64_t)n * levels[l].d * levels[l].h * levels[l].w + DS_FWD_PER_BLOCK - 1) / DS_FWD_PER_BLOCK;
        if (b > DS_FWD_CAP) b = DS_FWD_CAP;
        if (b < 1) b = 1;
        total += b;
    }
    return (int)total;
}

extern "C" size_t ru3d_ds_state_bytes(void) { return sizeof(DsState); }
extern "C" size_t ru3d_ds_state_bad_labels_offset(void) { return offsetof(DsState, lev) + offsetof(DsLevelState, bad_labels); }
extern "C" size_t ru3d_ds_block_bytes(void) { return (2 * RU3D_DS_MAX_LEVELS + 1) * sizeof(float); }

extern "C" size_t ru3d_ds_loss_workspace_bytes(const ru3d_ds_level* levels, int num_levels, int n) {
    if (!levels || num_levels < 1 || num_levels > RU3D_DS_MAX_LEVELS || n < 1) return 0;
    for (int l = 0; l < num_levels; l++)
        if (levels[l].d < 1 || levels[l].h < 1 || levels[l].w < 1) return 0;
    return (size_t)ds_fwd_blocks(levels, num_levels, n) * (4 * RU3D_MAX_CLASSES + 1) * sizeof(double);
}

#define DS_DISPATCH_C(C, CALL)   \
    switch (C) {                 \
        case 1: CALL(1); break;  \
        case 2: CALL(2); break;  \
        case 3: CALL(3); break;  \
        case 4: CALL(4); break;  \
        case 5: CALL(5); break;  \
        case 6: CALL(6); break;  \
        case 7: CALL(7); break;  \
        default: CALL(8); break; \
    }

extern "C" int ru3d_ds_loss_fwd(const ru3d_ds_level* levels, int num_levels, const void* labels, int label_dtype, int n,
                                int D, int H, int W, int num_classes, int kind, float gamma, const float* weight_v,
                                float alpha, float beta, float smooth, float* block, void* state, float* loss_out,
                                void* ws, size_t ws_bytes, void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    RU3D_REQUIRE(block && state && loss_out && ws, "ds_loss_fwd: null pointer");
    RU3D_REQUIRE(num_classes >= 1 && num_classes <= RU3D_MAX_CLASSES, "ds_loss_fwd: %d classes unsupported (max %d)",
                 num_classes, RU3D_MAX_CLASSES);
    RU3D_REQUIRE(kind == RU3D_LOSS_HYBIRD || kind == RU3D_LOSS_DICELOSS || kind == RU3D_LOSS_FOCAL,
                 "ds_loss_fwd: bad kind %d (HYBIRD, DICELOSS or FOCAL)", kind);
    DsArgs A;
    int rc = ds_fill_args(A, levels, nullptr, num_levels, labels, label_dtype, n, D, H, W, DS_FWD_PER_BLOCK, DS_FWD_CAP,
                          "ds_loss_fwd");
    if (rc) return rc;
    RU3D_REQUIRE(ws_bytes >= (size_t)A.nblocks * (4 * RU3D_MAX_CLASSES + 1) * sizeof(double),
                 "ds_loss_fwd: workspace too small");
    hipStream_t st = as_stream(stream);
#define CALL(CC) hipLaunchKernelGGL(ds_sums_kernel<CC>, dim3(A.nblocks), dim3(256), 0, st, A, gamma, (double*)ws)
    DS_DISPATCH_C(num_classes, CALL)
#undef CALL
    rc = ru3d_check_launch("ds_loss_sums");
    if (rc) return rc;
    DsParams P;
    P.kind = kind;
    P.C = num_classes;
    P.levels = num_levels;
    P.gamma = gamma;
    P.alpha = alpha;
    P.beta = beta;
    P.smooth = smooth;
    for (int c = 0; c < RU3D_MAX_CLASSES; c++) P.w[c] = (c < num_classes) ? (weight_v ? weight_v[c] : 1.f) : 0.f;
    for (int l = 0; l <= RU3D_DS_MAX_LEVELS; l++) P.blocks[l] = (l < num_levels) ? A.lev[l].block0 : A.nblocks;
    for (int l = 0; l < RU3D_DS_MAX_LEVELS; l++) P.nv[l] = (l < num_levels) ? (double)n * (double)A.lev[l].v : 1.0;
    hipLaunchKernelGGL(ds_finalize_kernel, dim3(1), dim3(DS_LF_THREADS), 0, st, (const double*)ws, P, block,
                       (DsState*)state, loss_out);
    return ru3d_check_launch("ds_loss_finalize");
}

extern "C" int ru3d_ds_loss_bwd(const ru3d_ds_level* levels, void* const* dlogits, int num_levels, const void* labels,
                                int label_dtype, int n, int D, int H, int W, int num_classes, float gamma,
                                const void* state, const float* grad_out, void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    RU3D_REQUIRE(state && dlogits, "ds_loss_bwd: null pointer");
    RU3D_REQUIRE(num_classes >= 1 && num_classes <= RU3D_MAX_CLASSES, "ds_loss_bwd: %d classes unsupported", num_classes);
    DsArgs A;
    int rc = ds_fill_args(A, levels, dlogits, num_levels, labels, label_dtype, n, D, H, W, DS_BWD_PER_BLOCK, DS_BWD_CAP,
                          "ds_loss_bwd");
    if (rc) return rc;
    hipStream_t st = as_stream(stream);
#define CALL(CC) \
    hipLaunchKernelGGL(ds_bwd_kernel<CC>, dim3(A.nblocks), dim3(256), 0, st, A, gamma, (const DsState*)state, grad_out)
    DS_DISPATCH_C(num_classes, CALL)
#undef CALL
    return ru3d_check_launch("ds_loss_bwd");
}
