// The one definition of what the fused losses share (loss.hip, deepsup.hip, groups.hip, topk.hip, cldice.hip,
// boundary.hip): the class limit and dispatch, the label load, the two softmax forms, and the region (softmax + focal +
// Tversky) loss piece by piece - per-voxel accumulate, block epilogue, fixed-order reduction of the partial rows, sums ->
// loss and backward coefficients, per-voxel backward - and, at the end, the host side of their entry points: grid rules,
// weight fill, argument checks, class list.  The formulas are restated in loss.hip's header.  Include this file beside
// common.h, BEFORE any `#pragma clang fp contract`: the multiply-add chains of the accumulate and of the backward are
// compiled under the default contraction.
#pragma once
#include "common.h"
#include <stddef.h>

#define RU3D_MAX_CLASSES 8

// CALL(C, ...) with the class count as a constant, MIN (1 or 2) .. 8; a file that rejects C == 1 passes MIN = 2 and gets
// no C = 1 kernel.  What follows CALL is handed on to it.
#define RU3D_DISPATCH_C1_FROM_1(CALL, ...) case 1: CALL(1, ##__VA_ARGS__); break;
#define RU3D_DISPATCH_C1_FROM_2(CALL, ...)
#define RU3D_DISPATCH_C(MIN, C, CALL, ...)                   \
    switch (C) {                                             \
        RU3D_DISPATCH_C1_FROM_##MIN(CALL, ##__VA_ARGS__)     \
        case 2: CALL(2, ##__VA_ARGS__); break;               \
        case 3: CALL(3, ##__VA_ARGS__); break;               \
        case 4: CALL(4, ##__VA_ARGS__); break;               \
        case 5: CALL(5, ##__VA_ARGS__); break;               \
        case 6: CALL(6, ##__VA_ARGS__); break;               \
        case 7: CALL(7, ##__VA_ARGS__); break;               \
        default: CALL(8, ##__VA_ARGS__); break;              \
    }
// CALL(C, TG) with TG the element type of a dlogits of DTYPE (RU3D_F32, else this build's 16-bit type)
#define RU3D_DISPATCH_C_DZ(MIN, C, DTYPE, CALL)  \
    if ((DTYPE) == RU3D_F32) {                   \
        RU3D_DISPATCH_C(MIN, C, CALL, float)     \
    } else {                                     \
        RU3D_DISPATCH_C(MIN, C, CALL, bf16)      \
    }

__device__ __forceinline__ int load_label(const void* labels, int label_dtype, int64_t i) {
    if (label_dtype == RU3D_LABEL_I64) return (int)((const int64_t*)labels)[i];
    return (int)((const uint8_t*)labels)[i];
}

// The ignore form of a loss kernel (template parameter IGN): a voxel whose label equals ignore_label is skipped before
// its logits are read - it enters no sum, its ce is 0, its gradient is written as exact zeros - so what its logits hold
// (NaN, Inf, padding) cannot reach anything.  Without IGN the test is compiled out.
template <bool IGN>
__device__ __forceinline__ bool label_ignored(int t, int ignore_label) {
    return IGN && t == ignore_label;
}

__device__ __forceinline__ float pow_gamma(float base, float gamma) {
    if (gamma == 2.f) return base * base;
    if (gamma == 1.f) return base;
    if (gamma == 0.f) return 1.f;
    return powf(base, gamma);
}

// log-softmax form: probabilities AND log-probabilities of one voxel, p = exp(lp) (sigmoid for C == 1)
template <int C>
__device__ __forceinline__ void voxel_probs(const float* __restrict__ z, int64_t stride_c, float (&p)[C],
                                            float (&lp)[C]) {
    float zz[C];
#pragma unroll
    for (int c = 0; c < C; c++) zz[c] = z[c * stride_c];
    if (C == 1) {
        // F.sigmoid / torch.log(pt)  (loss.py:227-228)
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

// e / sum e form: probabilities only (clDice, boundary).  Rounds differently from voxel_probs - not interchangeable.
template <int C>
__device__ __forceinline__ void softmax_probs(const float* __restrict__ z, int64_t stride_c, float (&p)[C]) {
    float zz[C];
#pragma unroll
    for (int c = 0; c < C; c++) zz[c] = z[c * stride_c];
    float m = zz[0];
#pragma unroll
    for (int c = 1; c < C; c++) m = fmaxf(m, zz[c]);
    float se = 0.f;
#pragma unroll
    for (int c = 0; c < C; c++) {
        p[c] = expf(zz[c] - m);
        se += p[c];
    }
    const float inv = 1.f / se;
#pragma unroll
    for (int c = 0; c < C; c++) p[c] *= inv;
}

// --------------------------------------------------------------------------- the region loss
// what a finalize leaves for the backward and for the host; LossState and deepsup's per-level state begin with it, so
// that bad_labels sits at one offset in every fused loss
struct RegionCoef {
    double sums[4][RU3D_MAX_CLASSES];  // tp, sp, sg, foc
    float qa[RU3D_MAX_CLASSES];        // dL/dp_c = qa_c * g_c + qb_c  (+ focal term)
    float qb[RU3D_MAX_CLASSES];
    float qf[RU3D_MAX_CLASSES];        // focal coefficient w_c * C / (N V)
    float loss;
    int bad_labels;
};
static_assert(sizeof(RegionCoef) == 360, "the state layouts of ru3d_loss_state_bytes / ru3d_ds_state_bytes are ABI");

constexpr int REGION_Q = 4 * RU3D_MAX_CLASSES + 1;  // one partial row: [4][MAX] sums, then the bad-label count
constexpr int REGION_LF_THREADS = 1024;             // workgroup of a finalize
constexpr int REGION_LF_GROUPS = REGION_LF_THREADS / REGION_Q;

// one voxel with label t into a thread's float32 partials of the forward
template <int C>
__device__ __forceinline__ void region_add(const float (&p)[C], const float (&lp)[C], int t, float gamma, float (&tp)[C],
                                           float (&sp)[C], float (&sg)[C], float (&fo)[C], int& bad) {
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
            fo[c] += -pow_gamma(1.f - p[c], gamma) * lp[c];
        }
    }
}

// block epilogue (256 threads): wave shuffles -> LDS -> this block's float64 partial row
template <int C>
__device__ __forceinline__ void region_write_row(const float (&tp)[C], const float (&sp)[C], const float (&sg)[C],
                                                 const float (&fo)[C], int bad, double* __restrict__ row) {
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
        const int dst = (q == 4 * C) ? 4 * RU3D_MAX_CLASSES : (q / C) * RU3D_MAX_CLASSES + (q % C);
        row[dst] = s;
    }
}

// tot[q] = sum of quantity q over `blocks` partial rows, by one workgroup of REGION_LF_THREADS: thread (g, q) sums the
// rows b = g, g + NG, ... (a wave-load covers consecutive q of one row: coalesced), then the NG group sums of a quantity
// are added in group order - fixed order, deterministic.  Ends with a barrier: every thread may read tot.
__device__ __forceinline__ void region_reduce_rows(const double* __restrict__ part, int blocks, int C,
                                                   double (&red)[REGION_LF_GROUPS][REGION_Q],
                                                   double (&tot)[REGION_Q]) {
    constexpr int Q = REGION_Q, NG = REGION_LF_GROUPS;
    const int g = threadIdx.x / Q, q = threadIdx.x % Q;
    if (g < NG) {
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
        int b = g;
        for (; b + 3 * NG < blocks; b += 4 * NG) {
            s0 += part[(int64_t)b * Q + q];
            s1 += part[(int64_t)(b + NG) * Q + q];
            s2 += part[(int64_t)(b + 2 * NG) * Q + q];
            s3 += part[(int64_t)(b + 3 * NG) * Q + q];
        }
        for (; b < blocks; b += NG) s0 += part[(int64_t)b * Q + q];
        red[g][q] = (s0 + s1) + (s2 + s3);
    }
    __syncthreads();
    if (threadIdx.x < Q) {
        const int qq = threadIdx.x, c = qq % RU3D_MAX_CLASSES;
        double t = 0.0;
        if (!(qq < 4 * RU3D_MAX_CLASSES && c >= C))
            for (int k = 0; k < NG; k++) t += red[k][qq];
        tot[qq] = t;
    }
    __syncthreads();
}

// One thread: the sums of tot -> the loss of `kind` (returned; NaN when `bad` labels were out of range - F.one_hot
// would have raised, loss.py:27) and everything of *st.  w_v: weight_v, un-normalised; NV: voxels of the batch.
__device__ __forceinline__ double region_coefficients(int kind, int C, const float* w_v, float alpha, float beta,
                                                      float smooth, double NV, const double* tot, int bad,
                                                      RegionCoef* __restrict__ st) {
    double wsum = 0.0;
    for (int c = 0; c < C; c++) wsum += fabs((double)w_v[c]);
    if (wsum < 1e-12) wsum = 1e-12;  // F.normalize eps
    const bool has_dice = kind != RU3D_LOSS_FOCAL;
    const bool has_focal = (kind == RU3D_LOSS_HYBIRD) || (kind == RU3D_LOSS_FOCAL);
    const double dsign = (kind == RU3D_LOSS_DICE) ? -1.0 : 1.0;  // loss = const - dsign * dice
    const double dconst = (kind == RU3D_LOSS_HYBIRD || kind == RU3D_LOSS_DICELOSS) ? 1.0 : 0.0;
    double loss = 0.0;
    for (int c = 0; c < RU3D_MAX_CLASSES; c++) {
        st->qa[c] = st->qb[c] = st->qf[c] = 0.f;
        for (int k = 0; k < 4; k++) st->sums[k][c] = tot[k * RU3D_MAX_CLASSES + c];
    }
    for (int c = 0; c < C; c++) {
        const double w = (double)w_v[c] / wsum;
        const double tp = tot[0 * RU3D_MAX_CLASSES + c], sp = tot[1 * RU3D_MAX_CLASSES + c],
                     sg = tot[2 * RU3D_MAX_CLASSES + c], fo = tot[3 * RU3D_MAX_CLASSES + c];
        double term = 0.0;
        if (has_dice) {
            const double a = alpha, b = beta, s = smooth;
            const double den = tp + a * (sg - tp) + b * (sp - tp) + s;
            const double dice = (tp + s) / den;
            term += dconst - dsign * dice;
            // d dice / d p_c(v) = g * A - B
            const double A = (den - (tp + s) * (1.0 - a - b)) / (den * den);
            const double B = (tp + s) * b / (den * den);
            st->qa[c] = (float)(-w * dsign * A);
            st->qb[c] = (float)(w * dsign * B);
        }
        if (has_focal) {
            term += (double)C * fo / NV;
            st->qf[c] = (float)(w * (double)C / NV);
        }
        loss += w * term;
    }
    st->bad_labels = bad;
    if (bad > 0) loss = nan("");
    st->loss = (float)loss;
    return loss;
}

// The voxel count of the focal mean.  Without an ignore label it is the batch's N V; with one it is M, the counted
// voxels: sum_c sg_c, float64 sums of exact small integers, floored at 1 (M = 0 leaves every sum 0: focal 0, dice 1).
template <bool IGN>
__device__ __forceinline__ double region_voxels(double NV, int C, const double* tot) {
    if (!IGN) return NV;
    double m = 0.0;
    for (int c = 0; c < C; c++) m += tot[2 * RU3D_MAX_CLASSES + c];
    return m < 1.0 ? 1.0 : m;
}

// the backward of one voxel: d[c] = d loss / d z_c from the coefficients a finalize left
template <int C>
struct RegionGrad {
    float qa[C], qb[C], qf[C];
    __device__ __forceinline__ explicit RegionGrad(const RegionCoef* __restrict__ st) {
#pragma unroll
        for (int c = 0; c < C; c++) {
            qa[c] = st->qa[c];
            qb[c] = st->qb[c];
            qf[c] = st->qf[c];
        }
    }
    __device__ __forceinline__ void voxel(const float (&p)[C], const float (&lp)[C], int t, float gamma,
                                          float (&d)[C]) const {
        float u[C], su = 0.f;
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
        for (int c = 0; c < C; c++) d[c] = (C == 1) ? u[0] * (1.f - p[0])  // sigmoid: dp/dz = p (1 - p)
                                                    : u[c] - p[c] * su;
    }
};

// --------------------------------------------------------------------------- host side of the entry points
// grid of a forward over `total` voxels: 8 voxels a thread, 256 threads, at most 2048 blocks (a block then strides)
static inline int region_fwd_blocks(int64_t total) {
    int64_t b = (total + 256 * 8 - 1) / (256 * 8);
    if (b > 2048) b = 2048;
    if (b < 1) b = 1;
    return (int)b;
}

// grid of a backward over `total` voxels: one voxel a thread, 256 threads, at most `cap` blocks
static inline int flat_bwd_blocks(int64_t total, int cap) {
    const int64_t b = (total + 255) / 256;
    return (int)(b < cap ? b : cap);
}

// w[k] = weight_v[index ? index[k] : k] for k < count (1 where the caller passed no weights), 0 behind
static inline void fill_class_weights(float (&w)[RU3D_MAX_CLASSES], const float* weight_v, int count,
                                      const int* index = nullptr) {
    for (int k = 0; k < RU3D_MAX_CLASSES; k++) w[k] = (k < count) ? (weight_v ? weight_v[index ? index[k] : k] : 1.f) : 0.f;
}

// The checks every entry point makes of its logits / labels view, in this order.  who: the entry point, for the
// message; pointers: the conjunction of its pointer arguments; nonempty: of its extents; count: classes (or `noun`),
// min_count .. RU3D_MAX_CLASSES.
static inline int loss_view_check(const char* who, bool pointers, bool nonempty, int label_dtype, int count,
                                  int min_count, const char* noun = "classes") {
    RU3D_REQUIRE(pointers, "%s: null pointer", who);
    RU3D_REQUIRE(nonempty, "%s: empty input", who);
    RU3D_REQUIRE(label_dtype == RU3D_LABEL_I64 || label_dtype == RU3D_LABEL_U8, "%s: bad label dtype", who);
    RU3D_REQUIRE(count >= min_count && count <= RU3D_MAX_CLASSES, "%s: %d %s unsupported (%d .. %d)", who, count, noun,
                 min_count, RU3D_MAX_CLASSES);
    return 0;
}

// The ignore label of the softmax losses, checked after loss_view_check and before any launch: it must not be a class,
// the single-channel (sigmoid) form has none, and uint8 labels can only carry 0 .. 255.
static inline int loss_ignore_check(const char* who, int has_ignore, int ignore_label, int label_dtype, int num_classes) {
    if (!has_ignore) return 0;
    RU3D_REQUIRE(num_classes >= 2, "%s: an ignore label needs at least 2 classes (the group loss is the single-channel form)", who);
    RU3D_REQUIRE(ignore_label < 0 || ignore_label >= num_classes, "%s: ignore_label %d is one of the %d classes", who,
                 ignore_label, num_classes);
    RU3D_REQUIRE(label_dtype != RU3D_LABEL_U8 || (ignore_label >= 0 && ignore_label <= 255),
                 "%s: uint8 labels cannot carry ignore_label %d", who, ignore_label);
    return 0;
}

// CALL(C, IGN, ...) for a run-time has_ignore: the ignore form is an instantiation of its own beside the plain one
#define RU3D_DISPATCH_C_IGN(MIN, C, HAS_IGNORE, CALL)  \
    if (HAS_IGNORE) {                                  \
        RU3D_DISPATCH_C(2, C, CALL, true)              \
    } else {                                           \
        RU3D_DISPATCH_C(MIN, C, CALL, false)           \
    }
#define RU3D_DISPATCH_C_DZ_IGN(MIN, C, DTYPE, HAS_IGNORE, CALL) \
    if ((DTYPE) == RU3D_F32) {                                   \
        if (HAS_IGNORE) {                                        \
            RU3D_DISPATCH_C(2, C, CALL, float, true)             \
        } else {                                                 \
            RU3D_DISPATCH_C(MIN, C, CALL, float, false)          \
        }                                                        \
    } else if (HAS_IGNORE) {                                     \
        RU3D_DISPATCH_C(2, C, CALL, bf16, true)                  \
    } else {                                                     \
        RU3D_DISPATCH_C(MIN, C, CALL, bf16, false)               \
    }

// the classes a loss is restricted to (clDice, boundary); goes to kernels by value
struct ClassList {
    int K;                          // selected classes
    int cls[RU3D_MAX_CLASSES];      // slot -> class
    int slot[RU3D_MAX_CLASSES];     // class -> slot, -1 when not selected
};

// num_classes has been checked (2 .. RU3D_MAX_CLASSES)
static inline int class_list_check(const char* what, int num_classes, const int* classes, int num_selected,
                                   ClassList* cl) {
    RU3D_REQUIRE(classes, "%s: null pointer (classes)", what);
    RU3D_REQUIRE(num_selected >= 1 && num_selected <= num_classes, "%s: bad class selection (num_selected = %d, 1 .. %d)",
                 what, num_selected, num_classes);
    cl->K = num_selected;
    for (int c = 0; c < RU3D_MAX_CLASSES; c++) {
        cl->cls[c] = 0;
        cl->slot[c] = -1;
    }
    for (int k = 0; k < num_selected; k++) {
        const int c = classes[k];
        RU3D_REQUIRE(c >= 0 && c < num_classes && cl->slot[c] < 0, "%s: class %d out of range or selected twice", what, c);
        cl->cls[k] = c;
        cl->slot[c] = k;
    }
    return 0;
}
