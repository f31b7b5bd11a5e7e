// Top-k cross-entropy on the device: exact top-K statistics of a flat float array (ru3d_topk_select) and the losses
// built on them (ru3d_topk_loss_fwd / _bwd: loss.TopKLoss, loss.HybirdTopKLoss - nnU-Net's DC_and_topk_loss).
//
// Definitions.  Logits (N, C, d1..dn), 2 <= C <= 8, labels (N, d1..dn), M = N * V voxels in the batch:
//   ce_v  = -log softmax(z_v)[t_v] in float32, from voxel_probs' lp (the arithmetic of the focal term); 0 for a voxel
//           whose label lies outside [0, C)
//   K     = max(1, int(M * k / 100)), computed once by the caller for 0 < k <= 100 and handed over as an int64
//   tau   = the K-th largest ce of the whole batch (the batch is flattened, as nnU-Net does)
//   G     = #{ce > tau},  E = #{ce == tau}
//   topk  = (sum_{ce > tau} ce + (K - G) * tau) / K             = torch.topk(ce, K).values.mean() whatever the ties
//   d topk / d z_{v,c} = s_v * (p_{v,c} - [c == t_v]) / K,  s_v = 1 if ce_v > tau, (K - G) / E if ce_v == tau, else 0:
//           the voxels tied at the threshold share the remaining weight equally, so the loss is deterministic and
//           independent of the voxel order; it is torch.topk's gradient whenever E == 1.  Ties at ce == 0 are real
//           (saturated voxels).
//   TopKLoss       = topk
//   HybirdTopKLoss = sum_c w_c (1 - dice_c) + ce_weight * topk,  w = weight_v / sum|weight_v| and the Tversky dice_c
//           exactly DiceLoss's (loss_core.h)
//   k = 100 is the plain mean cross-entropy.
//   With an ignore label (the IGN instantiations; nnU-Net's ignore_index rule): an ignored voxel has ce = 0 without its
//   logits being read, is selected like any voxel whose cross-entropy is 0 - K stays relative to all M voxels - and gets
//   a zero gradient whatever s_v the tie rule gives to ce == tau == 0; the Dice term sums over the counted voxels only.
//
// The select.  Radix select on select_key.h's order-preserving key, three digits of 11 / 11 / 10 bits, most significant
// first; the two zeros are one value (the key is taken of x + 0, and a zero tau is +0).  A level counts the digit of the
// values that share the digits chosen so far (LDS histogram of 2048 bins, integer atomics, one global integer add per
// non-empty bin and workgroup); one workgroup then walks the bins from the top and picks the one that holds the rank
// that is left, adding the counts above it to G.  The pass that counts digit l also sums, in float64 from the element
// on, the values that share the chosen digits 0 .. l-2 and whose digit l-1 lies strictly above the chosen bin: they are
// certainly inside the top K.  What lies above the picked bin of the LAST digit needs no pass at all: the last digit
// completes the key, a bin of its table holds copies of one value, and the workgroup that picks it adds count * value
// over the bins above.  So the values are read once per level; the loss counts the first digit while it writes ce[],
// which leaves two reads.  The sums go to per-workgroup partial rows that one workgroup adds in a fixed order: no float
// atomics, the same bits every run.  Nothing is sorted or moved, nothing comes back to the host, every launch is
// capturable.
//
// The backward compares the STORED ce with tau - it does not recompute the comparison operand, because two
// compilations of one expression need not round alike - so ce[] is the caller's buffer and lives until the backward.
#include "common.h"
#include "loss_core.h"
#include "bitvol.h"
#include "select_key.h"

#define TK_THREADS PP_THREADS
#define TK_WAVES (TK_THREADS / RU3D_WAVE)
#define TK_LEVELS 3
#define TK_BINS 2048                         // the widest digit: 11 bits, an 8 KB LDS table
#define TK_MAX_BLOCKS 1024                   // cap of the streaming grids; also the partial rows per level
#define TK_PICK_THREADS 256

typedef unsigned long long tk_u64;

__host__ __device__ constexpr int tk_shift(int level) { return level == 0 ? 21 : level == 1 ? 10 : 0; }
__host__ __device__ constexpr int tk_width(int level) { return level == 2 ? 10 : 11; }

// -0 and +0 are one value: x + 0 is +0 for both
__device__ __forceinline__ unsigned tk_key(float x) { return pp_key(x + 0.f); }

struct TkSelect {
    unsigned prefix;                         // the digits chosen so far, most significant first
    int bin;                                 // the last of them
    long long k_left;                        // the rank from the top that is left among the values sharing the prefix
    long long count_gt, count_eq;            // the values above the prefix so far; the values in the picked bin
};
static_assert(sizeof(ru3d_topk_result) == 32, "ru3d_topk_result is ABI");

// ++h[bin] for the active lanes; a wave whose lanes all meet one bin (a saturated batch: every ce is 0) sends one add
__device__ __forceinline__ void tk_lds_count(unsigned* h, unsigned bin) {
    const tk_u64 active = __ballot(1);
    const unsigned first = (unsigned)__builtin_amdgcn_readfirstlane((int)bin);
    if (__ballot(bin == first) == active) {
        if ((int)(threadIdx.x & 63) == __ffsll((long long)active) - 1) atomicAdd(&h[first], (unsigned)__popcll(active));
    } else {
        atomicAdd(&h[bin], 1u);
    }
}

__device__ __forceinline__ void tk_flush_hist(const unsigned* s_hist, tk_u64* __restrict__ hist) {
    for (int i = threadIdx.x; i < TK_BINS; i += TK_THREADS) {
        const unsigned c = s_hist[i];
        if (c) atomicAdd(hist + i, (tk_u64)c);
    }
}

__global__ __launch_bounds__(TK_THREADS) void tk_zero_kernel(tk_u64* __restrict__ hist, int count) {
    const int i = blockIdx.x * TK_THREADS + threadIdx.x;
    if (i < count) hist[i] = 0;
}

// level 0 of the stand-alone select: the top digit of every value
__global__ __launch_bounds__(TK_THREADS) void tk_hist0_kernel(const float* __restrict__ v, int64_t n,
                                                              tk_u64* __restrict__ hist) {
    __shared__ unsigned s_hist[TK_BINS];
    for (int i = threadIdx.x; i < TK_BINS; i += TK_THREADS) s_hist[i] = 0;
    __syncthreads();
    pp_stream<1>(v, n, [&](float x) { tk_lds_count(s_hist, tk_key(x) >> tk_shift(0)); });
    __syncthreads();
    tk_flush_hist(s_hist, hist);
}

// level 1 .. TK_LEVELS - 1: with P the digits 0 .. level-1 picked so far, count digit `level` of the values whose leading
// digits equal P, and sum those that share the digits 0 .. level-2 and lie above P in digit level-1.  rows[blockIdx.x]
// receives this workgroup's float64 sum.
__global__ __launch_bounds__(TK_THREADS) void tk_pass_kernel(const float* __restrict__ v, int64_t n, int level,
                                                             const TkSelect* __restrict__ st,
                                                             tk_u64* __restrict__ hist, double* __restrict__ rows) {
    __shared__ unsigned s_hist[TK_BINS];
    __shared__ double s_red[TK_WAVES];
    for (int i = threadIdx.x; i < TK_BINS; i += TK_THREADS) s_hist[i] = 0;
    const unsigned P = st->prefix;
    const int sp = tk_shift(level - 1), wp = tk_width(level - 1), sc = tk_shift(level);
    const unsigned mc = (1u << tk_width(level)) - 1u;
    __syncthreads();
    double s = 0.0;
    pp_stream<1>(v, n, [&](float x) {
        const unsigned key = tk_key(x), hi = key >> sp;
        if (hi == P)
            tk_lds_count(s_hist, (key >> sc) & mc);
        else if (hi > P && (hi >> wp) == (P >> wp))
            s += (double)x;
    });
    s = wave_sum_d(s);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) rows[blockIdx.x] = ((s_red[0] + s_red[1]) + s_red[2]) + s_red[3];
    tk_flush_hist(s_hist, hist);
}

// The pick of one level by a workgroup of at least TK_PICK_THREADS threads, all of which call it; thread t < 256 holds the
// bins 8 t .. 8 t + 7 of the level's table in h.  The bin, counted from the top, whose running count passes the rank k
// that is left: exactly one qualifies, the bins tile the ranks 1 .. (values sharing the prefix P).  *out (shared memory)
// is complete for every thread on return.
constexpr int TK_PER = TK_BINS / TK_PICK_THREADS;
__device__ __forceinline__ void tk_pick(int level, tk_u64 k, unsigned P, long long G, const tk_u64* __restrict__ hist,
                                        tk_u64 (&h)[TK_PER], tk_u64 (&s_cum)[TK_PICK_THREADS], TkSelect* out) {
    const int t = threadIdx.x;
    const bool mine = t < TK_PICK_THREADS;
    tk_u64 sum = 0;
#pragma unroll
    for (int j = 0; j < TK_PER; j++) {
        h[j] = mine ? hist[t * TK_PER + j] : 0;
        sum += h[j];
    }
    if (mine) s_cum[t] = sum;
    __syncthreads();
    for (int off = 1; off < TK_PICK_THREADS; off <<= 1) {
        const tk_u64 a = (mine && t >= off) ? s_cum[t - off] : 0;
        __syncthreads();
        if (mine) s_cum[t] += a;
        __syncthreads();
    }
    if (mine) {
        tk_u64 above = s_cum[TK_PICK_THREADS - 1] - s_cum[t];     // the values in the bins of the threads above this one
#pragma unroll
        for (int j = TK_PER - 1; j >= 0; j--) {
            if (h[j] != 0 && above < k && k <= above + h[j]) {
                out->bin = t * TK_PER + j;
                out->prefix = (P << tk_width(level)) | (unsigned)(t * TK_PER + j);
                out->k_left = (long long)(k - above);
                out->count_gt = G + (long long)above;
                out->count_eq = (long long)h[j];
            }
            above += h[j];
        }
    }
    __syncthreads();
}

// levels 0 .. TK_LEVELS - 2: one workgroup leaves the pick in *st for the pass that follows
__global__ __launch_bounds__(TK_PICK_THREADS) void tk_pick_kernel(int level, long long K, TkSelect* __restrict__ st,
                                                                  const tk_u64* __restrict__ hist) {
    __shared__ tk_u64 s_cum[TK_PICK_THREADS];
    __shared__ TkSelect picked;
    // every thread reads the state before the barriers of tk_pick, the one write comes after them
    const tk_u64 k = (tk_u64)(level == 0 ? K : st->k_left);
    const unsigned P = level == 0 ? 0u : st->prefix;
    const long long G = level == 0 ? 0 : st->count_gt;
    tk_u64 h[TK_PER];
    tk_pick(level, k, P, G, hist, h, s_cum, &picked);
    if (threadIdx.x == 0) *st = picked;
}

// The last level, inside the kernel that finishes (at least 256 threads, all of which call it): the pick, and the sum of
// the values that share the digits 0 .. TK_LEVELS-2 and lie above the picked bin - taken from the table, because the last
// digit completes the key: bin b holds h[b] copies of the one value pp_unkey(P b).  Thread t adds its own bins in
// ascending order, a tree adds the threads: a fixed order.  *picked (shared memory) is complete on return.
__device__ __forceinline__ double tk_pick_last(const TkSelect* __restrict__ st, const tk_u64* __restrict__ hist,
                                               tk_u64 (&s_cum)[TK_PICK_THREADS], double (&buf)[256], TkSelect* picked) {
    constexpr int LAST = TK_LEVELS - 1;
    const int t = threadIdx.x;
    const unsigned P = st->prefix;
    tk_u64 h[TK_PER];
    tk_pick(LAST, (tk_u64)st->k_left, P, st->count_gt, hist, h, s_cum, picked);
    if (t < 256) {
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < TK_PER; j++) {
            const int b = t * TK_PER + j;
            if (h[j] != 0 && b > picked->bin) s += (double)h[j] * (double)pp_unkey((P << tk_width(LAST)) | (unsigned)b);
        }
        buf[t] = s;
    }
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (t < off) buf[t] += buf[t + off];
        __syncthreads();
    }
    const double total = buf[0];
    __syncthreads();                         // buf is free again
    return total;
}

// sum of `count` partial rows by the first 256 threads of a workgroup, in a fixed order; every thread gets the total
__device__ __forceinline__ double tk_sum_rows(const double* __restrict__ rows, int count, double (&buf)[256]) {
    const int t = threadIdx.x;
    if (t < 256) {
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;     // four loads in flight; the order is fixed all the same
        int i = t;
        for (; i + 768 < count; i += 1024) {
            s0 += rows[i];
            s1 += rows[i + 256];
            s2 += rows[i + 512];
            s3 += rows[i + 768];
        }
        for (; i < count; i += 256) s0 += rows[i];
        buf[t] = (s0 + s1) + (s2 + s3);
    }
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (t < off) buf[t] += buf[t + off];
        __syncthreads();
    }
    const double total = buf[0];
    __syncthreads();                         // buf is free again
    return total;
}

__global__ __launch_bounds__(256) void tk_select_finish_kernel(const TkSelect* __restrict__ st,
                                                               const tk_u64* __restrict__ hist_last,
                                                               const double* __restrict__ rows, int count,
                                                               ru3d_topk_result* __restrict__ out) {
    __shared__ double buf[256];
    __shared__ tk_u64 s_cum[TK_PICK_THREADS];
    __shared__ TkSelect picked;
    const double last = tk_pick_last(st, hist_last, s_cum, buf, &picked);
    const double sum = tk_sum_rows(rows, count, buf);
    if (threadIdx.x != 0) return;
    out->tau = pp_unkey(picked.prefix);
    out->count_gt = picked.count_gt;
    out->count_eq = picked.count_eq;
    out->sum_gt = sum + last;
}

// --------------------------------------------------------------------------- workspace of a select
static unsigned tk_stream_blocks(int64_t n) {
    int64_t blocks = ((n + 3) / 4 + TK_THREADS - 1) / TK_THREADS;
    blocks = blocks > TK_MAX_BLOCKS ? TK_MAX_BLOCKS : blocks;
    return (unsigned)(blocks < 1 ? 1 : blocks);
}

struct TkWorkspace {
    TkSelect* st;
    tk_u64* hist;                            // [TK_LEVELS][TK_BINS]
    double* rows;                            // [TK_LEVELS - 1][blocks]
    unsigned blocks;
};
static size_t tk_select_bytes(int64_t n) {
    return bv_align(sizeof(TkSelect)) + bv_align((size_t)TK_LEVELS * TK_BINS * sizeof(tk_u64)) +
           bv_align((size_t)(TK_LEVELS - 1) * tk_stream_blocks(n) * sizeof(double));
}
static TkWorkspace tk_carve(void* ws, int64_t n) {
    TkWorkspace w;
    char* p = (char*)ws;
    w.st = (TkSelect*)p;
    p += bv_align(sizeof(TkSelect));
    w.hist = (tk_u64*)p;
    p += bv_align((size_t)TK_LEVELS * TK_BINS * sizeof(tk_u64));
    w.rows = (double*)p;
    w.blocks = tk_stream_blocks(n);
    return w;
}

static void tk_launch_zero(const TkWorkspace& w, hipStream_t st) {
    const int count = TK_LEVELS * TK_BINS;
    hipLaunchKernelGGL(tk_zero_kernel, dim3((count + TK_THREADS - 1) / TK_THREADS), dim3(TK_THREADS), 0, st, w.hist, count);
}

// the picks and the passes that follow the level-0 histogram, up to the table of the last digit; ev (tools only): an
// event after every launch
static void tk_launch_levels(const float* values, int64_t n, int64_t K, const TkWorkspace& w, hipStream_t st,
                             hipEvent_t* ev) {
    for (int level = 0; level + 1 < TK_LEVELS; level++) {
        hipLaunchKernelGGL(tk_pick_kernel, dim3(1), dim3(TK_PICK_THREADS), 0, st, level, (long long)K, w.st,
                           (const tk_u64*)(w.hist + (size_t)level * TK_BINS));
        if (ev) (void)hipEventRecord(*ev++, st);
        hipLaunchKernelGGL(tk_pass_kernel, dim3(w.blocks), dim3(TK_THREADS), 0, st, values, n, level + 1,
                           (const TkSelect*)w.st, w.hist + (size_t)(level + 1) * TK_BINS, w.rows + (size_t)level * w.blocks);
        if (ev) (void)hipEventRecord(*ev++, st);
    }
}

extern "C" size_t ru3d_topk_select_workspace_bytes(int64_t n) { return n >= 1 ? tk_select_bytes(n) : 0; }

extern "C" int64_t ru3d_topk_select_trip_elements(void) { return (int64_t)TK_MAX_BLOCKS * TK_THREADS * 4; }

extern "C" int ru3d_topk_select(const float* values, int64_t n, int64_t K, ru3d_topk_result* result, void* ws,
                                size_t ws_bytes, void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    RU3D_REQUIRE(n >= 1 && n < ((int64_t)1 << 40), "topk_select: %lld values (1 .. 2^40 - 1)", (long long)n);
    RU3D_REQUIRE(K >= 1 && K <= n, "topk_select: K = %lld of %lld values", (long long)K, (long long)n);
    RU3D_REQUIRE(values && result && ws, "topk_select: bad argument (null pointer)");
    RU3D_REQUIRE(((uintptr_t)values & 3) == 0, "topk_select: the values are not 4-byte aligned");
    RU3D_REQUIRE(((uintptr_t)result & 7) == 0 && ((uintptr_t)ws & 7) == 0, "topk_select: result or workspace not 8-byte aligned");
    RU3D_REQUIRE(ws_bytes >= tk_select_bytes(n), "topk_select: workspace of %zu bytes, %zu needed", ws_bytes,
                 tk_select_bytes(n));
    hipStream_t st = as_stream(stream);
    const TkWorkspace w = tk_carve(ws, n);
    tk_launch_zero(w, st);
    hipLaunchKernelGGL(tk_hist0_kernel, dim3(w.blocks), dim3(TK_THREADS), 0, st, values, n, w.hist);
    tk_launch_levels(values, n, K, w, st, nullptr);
    hipLaunchKernelGGL(tk_select_finish_kernel, dim3(1), dim3(256), 0, st, (const TkSelect*)w.st,
                       (const tk_u64*)(w.hist + (size_t)(TK_LEVELS - 1) * TK_BINS), (const double*)w.rows,
                       (int)((TK_LEVELS - 1) * w.blocks), result);
    return ru3d_check_launch("topk_select");
}

// --------------------------------------------------------------------------- the losses
struct TopKState {
    RegionCoef r;                            // first, so that bad_labels sits where every fused loss keeps it
    float tau;
    int pad;
    long long G, E, K;
    float w_gt;                              // ce_weight / K: the backward weight of a voxel with ce > tau
    float w_eq;                              // ce_weight * (K - G) / (E * K): of a voxel with ce == tau
};
static_assert(offsetof(TopKState, r) == 0 && sizeof(TopKState) == 400, "the state layout of ru3d_topk_loss_state_bytes is ABI");

extern "C" size_t ru3d_topk_loss_state_bytes(void) { return sizeof(TopKState); }

static size_t tk_region_bytes(int n, int64_t v) {
    return bv_align((size_t)region_fwd_blocks((int64_t)n * v) * REGION_Q * sizeof(double));
}

extern "C" size_t ru3d_topk_loss_workspace_bytes(int n, int64_t v, int num_classes) {
    (void)num_classes;
    if (n < 1 || v < 1) return 0;
    return tk_region_bytes(n, v) + tk_select_bytes((int64_t)n * v);
}

// the first pass: logits and labels read once; ce[] written, the top digit of every ce counted, and - with_dice - the
// region sums tp / sp / sg of the Tversky term.  part: one row of REGION_Q doubles per workgroup (the bad-label count
// is its last entry, with or without the region sums).
template <int C, bool IGN>
__global__ __launch_bounds__(256) void tk_ce_kernel(const float* __restrict__ logits, int64_t stride_n, int64_t stride_c,
                                                    int64_t stride_v, const void* __restrict__ labels, int label_dtype,
                                                    int n, int64_t v, int with_dice, int ignore_label,
                                                    float* __restrict__ ce,
                                                    tk_u64* __restrict__ hist, double* __restrict__ part) {
    __shared__ unsigned s_hist[TK_BINS];
    for (int i = threadIdx.x; i < TK_BINS; i += 256) s_hist[i] = 0;
    __syncthreads();
    float tp[C], sp[C], sg[C], fo[C];
#pragma unroll
    for (int c = 0; c < C; c++) tp[c] = sp[c] = sg[c] = fo[c] = 0.f;
    int bad = 0;
    const int64_t total = (int64_t)n * v;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t ni = i / v, vi = i - ni * v;
        const int t = load_label(labels, label_dtype, i);
        float cev = 0.f;                     // a label out of range, or the ignore label: ce = 0
        if (!label_ignored<IGN>(t, ignore_label)) {      // an ignored voxel enters the selection as a zero and no sum
            float p[C], lp[C];
            voxel_probs<C>(logits + ni * stride_n + vi * stride_v, stride_c, p, lp);
#pragma unroll
            for (int c = 0; c < C; c++)
                if (c == t) cev = 0.f - lp[c];   // lp <= 0; 0 - (+0) is +0, never -0
            if (with_dice)
                region_add<C>(p, lp, t, 0.f, tp, sp, sg, fo, bad);
            else
                bad += (t < 0 || t >= C);
        }
        ce[i] = cev;
        tk_lds_count(s_hist, tk_key(cev) >> tk_shift(0));
    }
    region_write_row<C>(tp, sp, sg, fo, bad, part + (int64_t)blockIdx.x * REGION_Q);
    __syncthreads();
    tk_flush_hist(s_hist, hist);
}

struct TkLossParams {
    int C, n, with_dice, sum_rows;
    int64_t v;
    long long K;
    float alpha, beta, smooth, ce_weight;
    float w[RU3D_MAX_CLASSES];               // weight_v (un-normalised); all ones when the caller passed NULL
};

__global__ __launch_bounds__(REGION_LF_THREADS) void tk_loss_finalize_kernel(const double* __restrict__ part, int blocks,
                                                                             const double* __restrict__ rows,
                                                                             TkLossParams P,
                                                                             const TkSelect* __restrict__ sel,
                                                                             const tk_u64* __restrict__ hist_last,
                                                                             TopKState* __restrict__ st,
                                                                             float* __restrict__ loss_out) {
    __shared__ double red[REGION_LF_GROUPS][REGION_Q];
    __shared__ double tot[REGION_Q];
    __shared__ double buf[256];
    __shared__ tk_u64 s_cum[TK_PICK_THREADS];
    __shared__ TkSelect picked;
    region_reduce_rows(part, blocks, P.C, red, tot);
    const double last = tk_pick_last(sel, hist_last, s_cum, buf, &picked);
    const double sum_gt = tk_sum_rows(rows, P.sum_rows, buf) + last;
    if (threadIdx.x != 0) return;
    const int bad = (int)tot[4 * RU3D_MAX_CLASSES];
    double loss = 0.0;
    if (P.with_dice) {
        loss = region_coefficients(RU3D_LOSS_DICELOSS, P.C, P.w, P.alpha, P.beta, P.smooth, (double)P.n * (double)P.v,
                                   tot, bad, &st->r);
    } else {
        for (int c = 0; c < RU3D_MAX_CLASSES; c++) {
            st->r.qa[c] = st->r.qb[c] = st->r.qf[c] = 0.f;
            for (int k = 0; k < 4; k++) st->r.sums[k][c] = 0.0;
        }
        st->r.bad_labels = bad;
    }
    const float tau32 = pp_unkey(picked.prefix);
    const double tau = (double)tau32, K = (double)P.K;
    const long long G = picked.count_gt, E = picked.count_eq;
    loss += (double)P.ce_weight * ((sum_gt + (double)(P.K - G) * tau) / K);
    if (bad > 0) loss = nan("");
    st->r.loss = (float)loss;
    st->tau = tau32;
    st->G = G;
    st->E = E;
    st->K = P.K;
    st->w_gt = (float)((double)P.ce_weight / K);
    st->w_eq = (float)((double)P.ce_weight * (double)(P.K - G) / ((double)E * K));
    st->pad = 0;
    loss_out[0] = (float)loss;
}

template <int C, typename TG, bool IGN>
__global__ __launch_bounds__(256) void tk_bwd_kernel(const float* __restrict__ logits, int64_t stride_n, int64_t stride_c,
                                                     int64_t stride_v, const void* __restrict__ labels, int label_dtype,
                                                     int n, int64_t v, int with_dice, int ignore_label,
                                                     const float* __restrict__ ce,
                                                     const TopKState* __restrict__ st, const float* __restrict__ grad_out,
                                                     TG* __restrict__ dz) {
    const RegionGrad<C> grad(&st->r);
    const float tau = st->tau, w_gt = st->w_gt, w_eq = st->w_eq;
    const float go = grad_out ? grad_out[0] : 1.f;
    const int64_t total = (int64_t)n * v;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t ni = i / v, vi = i - ni * v;
        const int64_t base = ni * stride_n + vi * stride_v;
        const int t = load_label(labels, label_dtype, i);
        if (label_ignored<IGN>(t, ignore_label)) {      // zero whatever share the tie rule gives to ce == tau == 0
#pragma unroll
            for (int c = 0; c < C; c++) dz[base + c * stride_c] = from_f32<TG>(0.f);
            continue;
        }
        float p[C], lp[C], d[C];
        voxel_probs<C>(logits + base, stride_c, p, lp);
        if (with_dice) {
            grad.voxel(p, lp, t, 0.f, d);
        } else {
#pragma unroll
            for (int c = 0; c < C; c++) d[c] = 0.f;
        }
        const float cev = ce[i];             // the stored value: the operand the select saw
        float s = cev > tau ? w_gt : (cev == tau ? w_eq : 0.f);
        if (t < 0 || t >= C) s = 0.f;
#pragma unroll
        for (int c = 0; c < C; c++) dz[base + c * stride_c] = from_f32<TG>((d[c] + s * (p[c] - (c == t ? 1.f : 0.f))) * go);
    }
}

#define TK_FWD_LAUNCHES (2 + 2 * (TK_LEVELS - 1) + 1)

static int tk_loss_forward(const float* logits, int64_t stride_n, int64_t stride_c, int64_t stride_v, const void* labels,
                           int label_dtype, int n, int64_t v, int num_classes, int has_ignore, int ignore_label,
                           int64_t K, int with_dice,
                           const float* weight_v, float alpha, float beta, float smooth, float ce_weight, float* ce,
                           void* state, float* loss_out, void* ws, size_t ws_bytes, void* stream, hipEvent_t* ev) {
    int rc = loss_view_check("topk_loss_fwd", logits && labels && ce && state && loss_out && ws, n > 0 && v > 0,
                             label_dtype, num_classes, 2);
    if (rc) return rc;
    rc = loss_ignore_check("topk_loss_fwd", has_ignore, ignore_label, label_dtype, num_classes);
    if (rc) return rc;
    const int64_t m = (int64_t)n * v;
    RU3D_REQUIRE(K >= 1 && K <= m, "topk_loss_fwd: K = %lld of %lld voxels", (long long)K, (long long)m);
    RU3D_REQUIRE(((uintptr_t)ce & 3) == 0 && ((uintptr_t)ws & 7) == 0 && ((uintptr_t)state & 7) == 0,
                 "topk_loss_fwd: ce, workspace or state misaligned");
    RU3D_REQUIRE(ws_bytes >= ru3d_topk_loss_workspace_bytes(n, v, num_classes), "topk_loss_fwd: workspace too small");
    hipStream_t st = as_stream(stream);
    const int blocks = region_fwd_blocks(m);
    double* part = (double*)ws;
    const TkWorkspace w = tk_carve((char*)ws + tk_region_bytes(n, v), m);
    if (ev) (void)hipEventRecord(*ev++, st);
    tk_launch_zero(w, st);
    if (ev) (void)hipEventRecord(*ev++, st);
#define CALL(CC, IGN)                                                                                               \
    hipLaunchKernelGGL((tk_ce_kernel<CC, IGN>), dim3(blocks), dim3(256), 0, st, logits, stride_n, stride_c, stride_v, \
                       labels, label_dtype, n, v, with_dice, ignore_label, ce, w.hist, part)
    RU3D_DISPATCH_C_IGN(2, num_classes, has_ignore, CALL)
#undef CALL
    if (ev) (void)hipEventRecord(*ev++, st);
    rc = ru3d_check_launch("topk_loss_ce");
    if (rc) return rc;
    tk_launch_levels(ce, m, K, w, st, ev);
    if (ev) ev += 2 * (TK_LEVELS - 1);
    TkLossParams P;
    P.C = num_classes;
    P.n = n;
    P.with_dice = with_dice != 0;
    P.sum_rows = (int)((TK_LEVELS - 1) * w.blocks);
    P.v = v;
    P.K = K;
    P.alpha = alpha;
    P.beta = beta;
    P.smooth = smooth;
    P.ce_weight = ce_weight;
    fill_class_weights(P.w, weight_v, num_classes);
    hipLaunchKernelGGL(tk_loss_finalize_kernel, dim3(1), dim3(REGION_LF_THREADS), 0, st, (const double*)part, blocks,
                       (const double*)w.rows, P, (const TkSelect*)w.st,
                       (const tk_u64*)(w.hist + (size_t)(TK_LEVELS - 1) * TK_BINS), (TopKState*)state, loss_out);
    if (ev) (void)hipEventRecord(*ev++, st);
    return ru3d_check_launch("topk_loss_finalize");
}

extern "C" int ru3d_topk_loss_ignore_fwd(const float* logits, int64_t stride_n, int64_t stride_c, int64_t stride_v,
                                         const void* labels, int label_dtype, int n, int64_t v, int num_classes,
                                         int has_ignore, int ignore_label, int64_t K, int with_dice,
                                         const float* weight_v, float alpha, float beta, float smooth, float ce_weight,
                                         float* ce, void* state, float* loss_out, void* ws, size_t ws_bytes,
                                         void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    return tk_loss_forward(logits, stride_n, stride_c, stride_v, labels, label_dtype, n, v, num_classes, has_ignore,
                           ignore_label, K, with_dice, weight_v, alpha, beta, smooth, ce_weight, ce, state, loss_out, ws,
                           ws_bytes, stream, nullptr);
}

extern "C" int ru3d_topk_loss_fwd(const float* logits, int64_t stride_n, int64_t stride_c, int64_t stride_v,
                                  const void* labels, int label_dtype, int n, int64_t v, int num_classes, int64_t K,
                                  int with_dice, const float* weight_v, float alpha, float beta, float smooth,
                                  float ce_weight, float* ce, void* state, float* loss_out, void* ws, size_t ws_bytes,
                                  void* stream) {
    return ru3d_topk_loss_ignore_fwd(logits, stride_n, stride_c, stride_v, labels, label_dtype, n, v, num_classes, 0, 0, K,
                                     with_dice, weight_v, alpha, beta, smooth, ce_weight, ce, state, loss_out, ws,
                                     ws_bytes, stream);
}

extern "C" int ru3d_topk_loss_fwd_launches(void) { return TK_FWD_LAUNCHES; }

// tools: the forward with an event after every launch; waits for the stream and writes the milliseconds of the
// ru3d_topk_loss_fwd_launches() launches, in launch order (clear, ce + first histogram, then the pick of a level and the
// pass of the next, finalize with the last pick), to the HOST array launch_ms.  Not capturable.
extern "C" int ru3d_topk_loss_fwd_timed(const float* logits, int64_t stride_n, int64_t stride_c, int64_t stride_v,
                                        const void* labels, int label_dtype, int n, int64_t v, int num_classes,
                                        int64_t K, int with_dice, const float* weight_v, float alpha, float beta,
                                        float smooth, float ce_weight, float* ce, void* state, float* loss_out, void* ws,
                                        size_t ws_bytes, float* launch_ms, void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    RU3D_REQUIRE(launch_ms, "topk_loss_fwd_timed: null pointer");
    hipEvent_t ev[TK_FWD_LAUNCHES + 1];
    int made = 0;
    for (; made <= TK_FWD_LAUNCHES; made++)
        if (hipEventCreate(&ev[made]) != hipSuccess) break;
    int rc = made == TK_FWD_LAUNCHES + 1 ? 0 : ru3d_fail(-1, "topk_loss_fwd_timed: hipEventCreate failed");
    if (!rc)
        rc = tk_loss_forward(logits, stride_n, stride_c, stride_v, labels, label_dtype, n, v, num_classes, 0, 0, K, with_dice,
                             weight_v, alpha, beta, smooth, ce_weight, ce, state, loss_out, ws, ws_bytes, stream, ev);
    if (!rc && hipEventSynchronize(ev[TK_FWD_LAUNCHES]) != hipSuccess)
        rc = ru3d_fail(-1, "topk_loss_fwd_timed: hipEventSynchronize failed");
    for (int i = 0; !rc && i < TK_FWD_LAUNCHES; i++)
        if (hipEventElapsedTime(&launch_ms[i], ev[i], ev[i + 1]) != hipSuccess)
            rc = ru3d_fail(-1, "topk_loss_fwd_timed: hipEventElapsedTime failed");
    for (int i = 0; i < made; i++) (void)hipEventDestroy(ev[i]);
    return rc;
}

extern "C" int ru3d_topk_loss_ignore_bwd(const float* logits, int64_t stride_n, int64_t stride_c, int64_t stride_v,
                                         const void* labels, int label_dtype, int n, int64_t v, int num_classes,
                                         int has_ignore, int ignore_label, int with_dice, const float* ce,
                                         const void* state, const float* grad_out, void* dlogits, int dlogits_dtype,
                                         void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    int rc = loss_view_check("topk_loss_bwd", logits && labels && ce && state && dlogits, n > 0 && v > 0, label_dtype,
                             num_classes, 2);
    if (rc) return rc;
    rc = loss_ignore_check("topk_loss_bwd", has_ignore, ignore_label, label_dtype, num_classes);
    if (rc) return rc;
    RU3D_REQUIRE(dlogits_dtype == RU3D_F32 || dlogits_dtype == RU3D_BF16, "topk_loss_bwd: bad dlogits dtype");
    hipStream_t st = as_stream(stream);
    const int blocks = flat_bwd_blocks((int64_t)n * v, 8192);
#define CALL(CC, TG, IGN)                                                                                           \
    hipLaunchKernelGGL((tk_bwd_kernel<CC, TG, IGN>), dim3(blocks), dim3(256), 0, st, logits, stride_n, stride_c,        \
                       stride_v, labels, label_dtype, n, v, with_dice, ignore_label, ce, (const TopKState*)state, grad_out, \
                       (TG*)dlogits)
    RU3D_DISPATCH_C_DZ_IGN(2, num_classes, dlogits_dtype, has_ignore, CALL)
#undef CALL
    return ru3d_check_launch("topk_loss_bwd");
}

extern "C" int ru3d_topk_loss_bwd(const float* logits, int64_t stride_n, int64_t stride_c, int64_t stride_v,
                                  const void* labels, int label_dtype, int n, int64_t v, int num_classes, int with_dice,
                                  const float* ce, const void* state, const float* grad_out, void* dlogits,
                                  int dlogits_dtype, void* stream) {
    return ru3d_topk_loss_ignore_bwd(logits, stride_n, stride_c, stride_v, labels, label_dtype, n, v, num_classes, 0, 0,
                                     with_dice, ce, state, grad_out, dlogits, dlogits_dtype, stream);
}
