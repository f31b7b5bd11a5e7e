// Deep supervision: the fused softmax + focal + Tversky loss of loss.hip on EVERY supervised decoder level at once - one
// sums launch and one finalize for all levels, one backward launch for all levels - against ONE full-resolution label
// tensor.  Level l (shift s) never gets labels of its own: voxel (a, b, c) of that level reads label[a << s][b << s][c << s]
// (label[:, ::2**s, ::2**s, ::2**s]: nearest-neighbour down-sampling with the integer step 2**s).
//
// The arithmetic and precisions are loss_core.h's, shared with loss.hip's single-tensor kernels, level by level: float32 per
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
#include "loss_core.h"

// per level: the region loss's coefficients first, so that level 0's count of out-of-range labels (no other level counts)
// sits where every fused loss keeps it
struct DsLevelState {
    RegionCoef r;
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

template <int C, bool IGN>
__global__ __launch_bounds__(256) void ds_sums_kernel(DsArgs A, float gamma, int ignore_label,
                                                      double* __restrict__ part) {
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
        const int t = load_label(A.labels, A.label_dtype, ds_label_index(A, Lv, ni, vi));
        if (label_ignored<IGN>(t, ignore_label)) continue;      // the level ignores a voxel iff the label it reads is ignored
        float p[C], lp[C];
        voxel_probs<C>(Lv.logits + ni * Lv.stride_n + vi * Lv.stride_v, Lv.stride_c, p, lp);
        region_add<C>(p, lp, t, gamma, tp, sp, sg, fo, bad);
    }
    region_write_row<C>(tp, sp, sg, fo, bad, part + (int64_t)blockIdx.x * REGION_Q);
}

// One workgroup of REGION_LF_THREADS, level after level: the fixed-order reduction of the level's partial rows, then
// thread 0 turns the sums into the level's loss and backward coefficients.  block: float32 [0 .. 7] the level weights
// (read), [8 .. 15] the levels' losses and [16] the total (written).
template <bool IGN>
__global__ __launch_bounds__(REGION_LF_THREADS) void ds_finalize_kernel(const double* __restrict__ part, DsParams P,
                                                                        float* __restrict__ block, DsState* __restrict__ st,
                                                                        float* __restrict__ loss_out) {
    __shared__ double red[REGION_LF_GROUPS][REGION_Q];
    __shared__ double tot[REGION_Q];
    double total = 0.0;      // thread 0's
    for (int l = 0; l < P.levels; l++) {
        region_reduce_rows(part + (int64_t)P.blocks[l] * REGION_Q, P.blocks[l + 1] - P.blocks[l], P.C, red, tot);
        if (threadIdx.x == 0) {
            DsLevelState* sl = &st->lev[l];
            // out-of-range labels are counted where every label is read once: on level 0
            const int bad = (l == 0) ? (int)tot[4 * RU3D_MAX_CLASSES] : 0;
            const double nv = region_voxels<IGN>(P.nv[l], P.C, tot);      // with an ignore label: the level's own M_l
            const double loss = region_coefficients(P.kind, P.C, P.w, P.alpha, P.beta, P.smooth, nv, tot, bad, &sl->r);
            const float wl = block[l];
            sl->weight = wl;
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

template <int C, bool IGN>
__global__ __launch_bounds__(256) void ds_bwd_kernel(DsArgs A, float gamma, int ignore_label,
                                                     const DsState* __restrict__ st,
                                                     const float* __restrict__ grad_out) {
    const int l = ds_level_of(A, blockIdx.x);
    const DsLevelArg Lv = A.lev[l];
    const int first = Lv.block0;
    const int count = ((l + 1 < A.levels) ? A.lev[l + 1].block0 : A.nblocks) - first;
    const DsLevelState* sl = &st->lev[l];
    const RegionGrad<C> grad(&sl->r);
    const float go = (grad_out ? grad_out[0] : 1.f) * sl->weight;
    const int64_t total = (int64_t)A.n * Lv.v;
    for (int64_t i = (int64_t)(blockIdx.x - first) * 256 + threadIdx.x; i < total; i += (int64_t)count * 256) {
        const int64_t ni = i / Lv.v, vi = i - ni * Lv.v;
        const int64_t base = ni * Lv.stride_n + vi * Lv.stride_v;
        const int t = load_label(A.labels, A.label_dtype, ds_label_index(A, Lv, ni, vi));
        if (label_ignored<IGN>(t, ignore_label)) {      // dlogits is uninitialised memory: the zeros are written
#pragma unroll
            for (int c = 0; c < C; c++) Lv.dlogits[base + c * Lv.stride_c] = 0.f;
            continue;
        }
        float p[C], lp[C], d[C];
        voxel_probs<C>(Lv.logits + base, Lv.stride_c, p, lp);
        grad.voxel(p, lp, t, gamma, d);
#pragma unroll
        for (int c = 0; c < C; c++) Lv.dlogits[base + c * Lv.stride_c] = d[c] * go;
    }
}

// the levels' block ranges: level l gets blocks_of(n v_l) blocks (a block strides over its level where that is capped);
// the caller has made loss_view_check
static int ds_fill_args(DsArgs& A, const ru3d_ds_level* levels, void* const* dlogits, int num_levels, const void* labels,
                        int label_dtype, int n, int D, int H, int W, int (*blocks_of)(int64_t), const char* what) {
    RU3D_REQUIRE(num_levels >= 1 && num_levels <= RU3D_DS_MAX_LEVELS, "%s: %d levels (1 .. %d)", what, num_levels,
                 RU3D_DS_MAX_LEVELS);
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
        next += blocks_of((int64_t)n * Lv.v);
    }
    A.nblocks = (int)next;
    return 0;
}

// the backward: 512 voxels a block (two trips of its 256 threads), at most 8192 blocks a level.  ceil(total / 512) is
// ceil(ceil(total / 2) / 256), and it is at least 1 because the entry point has refused total < 1.
static int ds_bwd_blocks(int64_t total) { return flat_bwd_blocks((total + 1) / 2, 8192); }

static int ds_fwd_blocks(const ru3d_ds_level* levels, int num_levels, int n) {
    int64_t total = 0;
    for (int l = 0; l < num_levels; l++) total += region_fwd_blocks((int64_t)n * levels[l].d * levels[l].h * levels[l].w);
    return (int)total;
}

extern "C" size_t ru3d_ds_state_bytes(void) { return sizeof(DsState); }
extern "C" size_t ru3d_ds_state_bad_labels_offset(void) { return offsetof(DsState, lev) + offsetof(DsLevelState, r) + offsetof(RegionCoef, bad_labels); }
extern "C" size_t ru3d_ds_block_bytes(void) { return (2 * RU3D_DS_MAX_LEVELS + 1) * sizeof(float); }

extern "C" size_t ru3d_ds_loss_workspace_bytes(const ru3d_ds_level* levels, int num_levels, int n) {
    if (!levels || num_levels < 1 || num_levels > RU3D_DS_MAX_LEVELS || n < 1) return 0;
    for (int l = 0; l < num_levels; l++)
        if (levels[l].d < 1 || levels[l].h < 1 || levels[l].w < 1) return 0;
    return (size_t)ds_fwd_blocks(levels, num_levels, n) * REGION_Q * sizeof(double);
}

extern "C" int ru3d_ds_loss_ignore_fwd(const ru3d_ds_level* levels, int num_levels, const void* labels, int label_dtype,
                                       int n, int D, int H, int W, int num_classes, int has_ignore, int ignore_label,
                                       int kind, float gamma, const float* weight_v, float alpha, float beta, float smooth,
                                       float* block, void* state, float* loss_out, void* ws, size_t ws_bytes,
                                       void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    int rc = loss_view_check("ds_loss_fwd", levels && labels && block && state && loss_out && ws,
                             n > 0 && D > 0 && H > 0 && W > 0, label_dtype, num_classes, 1);
    if (rc) return rc;
    rc = loss_ignore_check("ds_loss_fwd", has_ignore, ignore_label, label_dtype, num_classes);
    if (rc) return rc;
    RU3D_REQUIRE(kind == RU3D_LOSS_HYBIRD || kind == RU3D_LOSS_DICELOSS || kind == RU3D_LOSS_FOCAL,
                 "ds_loss_fwd: bad kind %d (HYBIRD, DICELOSS or FOCAL)", kind);
    DsArgs A;
    rc = ds_fill_args(A, levels, nullptr, num_levels, labels, label_dtype, n, D, H, W, region_fwd_blocks, "ds_loss_fwd");
    if (rc) return rc;
    RU3D_REQUIRE(ws_bytes >= (size_t)A.nblocks * REGION_Q * sizeof(double),
                 "ds_loss_fwd: workspace too small");
    hipStream_t st = as_stream(stream);
#define CALL(CC, IGN) \
    hipLaunchKernelGGL((ds_sums_kernel<CC, IGN>), dim3(A.nblocks), dim3(256), 0, st, A, gamma, ignore_label, (double*)ws)
    RU3D_DISPATCH_C_IGN(1, num_classes, has_ignore, CALL)
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
    fill_class_weights(P.w, weight_v, num_classes);
    for (int l = 0; l <= RU3D_DS_MAX_LEVELS; l++) P.blocks[l] = (l < num_levels) ? A.lev[l].block0 : A.nblocks;
    for (int l = 0; l < RU3D_DS_MAX_LEVELS; l++) P.nv[l] = (l < num_levels) ? (double)n * (double)A.lev[l].v : 1.0;
    if (has_ignore)
        hipLaunchKernelGGL(ds_finalize_kernel<true>, dim3(1), dim3(REGION_LF_THREADS), 0, st, (const double*)ws, P, block,
                           (DsState*)state, loss_out);
    else
        hipLaunchKernelGGL(ds_finalize_kernel<false>, dim3(1), dim3(REGION_LF_THREADS), 0, st, (const double*)ws, P, block,
                           (DsState*)state, loss_out);
    return ru3d_check_launch("ds_loss_finalize");
}

extern "C" int ru3d_ds_loss_fwd(const ru3d_ds_level* levels, int num_levels, const void* labels, int label_dtype, int n,
                                int D, int H, int W, int num_classes, int kind, float gamma, const float* weight_v,
                                float alpha, float beta, float smooth, float* block, void* state, float* loss_out,
                                void* ws, size_t ws_bytes, void* stream) {
    return ru3d_ds_loss_ignore_fwd(levels, num_levels, labels, label_dtype, n, D, H, W, num_classes, 0, 0, kind, gamma,
                                   weight_v, alpha, beta, smooth, block, state, loss_out, ws, ws_bytes, stream);
}

extern "C" int ru3d_ds_loss_ignore_bwd(const ru3d_ds_level* levels, void* const* dlogits, int num_levels,
                                       const void* labels, int label_dtype, int n, int D, int H, int W, int num_classes,
                                       int has_ignore, int ignore_label, float gamma, const void* state,
                                       const float* grad_out, void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    int rc = loss_view_check("ds_loss_bwd", levels && labels && state && dlogits, n > 0 && D > 0 && H > 0 && W > 0,
                             label_dtype, num_classes, 1);
    if (rc) return rc;
    rc = loss_ignore_check("ds_loss_bwd", has_ignore, ignore_label, label_dtype, num_classes);
    if (rc) return rc;
    DsArgs A;
    rc = ds_fill_args(A, levels, dlogits, num_levels, labels, label_dtype, n, D, H, W, ds_bwd_blocks, "ds_loss_bwd");
    if (rc) return rc;
    hipStream_t st = as_stream(stream);
#define CALL(CC, IGN)                                                                                            \
    hipLaunchKernelGGL((ds_bwd_kernel<CC, IGN>), dim3(A.nblocks), dim3(256), 0, st, A, gamma, ignore_label, \
                       (const DsState*)state, grad_out)
    RU3D_DISPATCH_C_IGN(1, num_classes, has_ignore, CALL)
#undef CALL
    return ru3d_check_launch("ds_loss_bwd");
}

extern "C" int ru3d_ds_loss_bwd(const ru3d_ds_level* levels, void* const* dlogits, int num_levels, const void* labels,
                                int label_dtype, int n, int D, int H, int W, int num_classes, float gamma,
                                const void* state, const float* grad_out, void* stream) {
    return ru3d_ds_loss_ignore_bwd(levels, dlogits, num_levels, labels, label_dtype, n, D, H, W, num_classes, 0, 0, gamma,
                                   state, grad_out, stream);
}
