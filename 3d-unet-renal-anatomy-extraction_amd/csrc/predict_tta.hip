// Sliding-window inference with test-time mirroring and centre-weighted blending (inference.py, the paths
// behind placement / weighting / mirror_axes / model lists).
//
// Two streaming passes around the model forward, both HBM-bound, no LDS, no atomics:
//   gather:      padded volume [X, Y, Z, Cin] fp32 -> the NDHWC model input [B, px, py, pz, Cin] fp32, every batch
//                entry with its own window origin and its own 3-bit mirror mask (bit 0 = X, 1 = Y, 2 = Z).  The mirror
//                is index arithmetic on the read side; the write side is dense.  The entries travel in the kernel
//                arguments and a block works on one entry (blockIdx.y), so the entry is read with scalar loads.
//   accumulate:  one batch entry of the logits -> softmax / sigmoid exactly as predict_accumulate_kernel, read at the
//                mirrored index (which puts the probabilities back on the volume's grid), times the separable weight
//                (g_x[a] * g_y[j]) * g_z[k] from three small fp32 tables, added into acc [X, Y, Z, C]; the weight is
//                added into cnt.  Null tables = weight 1, then the arithmetic is the plain add of
//                predict_accumulate_kernel.  A launch touches every voxel of its window once (read-modify-write by one
//                thread), overlapping windows are ordered by the stream: the sum order is the launch order.
// Mirrored reads run backwards along an axis; a wave still touches one contiguous span, so they stay coalesced.
#include "common.h"

#define RU3D_PREDICT_MAX_CLASSES 8

struct GatherEntries {
    int ox[RU3D_PREDICT_MAX_BATCH], oy[RU3D_PREDICT_MAX_BATCH], oz[RU3D_PREDICT_MAX_BATCH], flip[RU3D_PREDICT_MAX_BATCH];
};

// generic: one thread per destination element, channel fastest
__global__ __launch_bounds__(256) void predict_gather_kernel(const float* __restrict__ vol, int Y, int Z, int cin,
                                                             float* __restrict__ dst, int px, int py, int pz,
                                                             GatherEntries e) {
    const int b = blockIdx.y;
    const int ox = e.ox[b], oy = e.oy[b], oz = e.oz[b], flip = e.flip[b];
    const int64_t total = (int64_t)px * py * pz * cin;
    float* out = dst + (int64_t)b * total;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int c = (int)(i % cin);
        int64_t r = i / cin;
        const int k = (int)(r % pz);
        r /= pz;
        const int j = (int)(r % py);
        const int a = (int)(r / py);
        const int sa = (flip & 1) ? px - 1 - a : a;
        const int sj = (flip & 2) ? py - 1 - j : j;
        const int sk = (flip & 4) ? pz - 1 - k : k;
        out[i] = vol[(((int64_t)(ox + sa) * Y + (oy + sj)) * Z + (oz + sk)) * cin + c];
    }
}

// Cin == 1, pz % 4 == 0, and every window row 16-byte aligned in the volume (Z % 4 == 0, oz % 4 == 0): 4 voxels of
// the z axis per thread as one 16-byte load and one 16-byte store; a z mirror reverses the four lanes of the load.
__global__ __launch_bounds__(256) void predict_gather_c1v4_kernel(const float* __restrict__ vol, int Y, int Z,
                                                                  float* __restrict__ dst, int px, int py, int pz,
                                                                  GatherEntries e) {
    const int b = blockIdx.y;
    const int ox = e.ox[b], oy = e.oy[b], oz = e.oz[b], flip = e.flip[b];
    const int qz = pz >> 2;
    const int64_t total = (int64_t)px * py * qz;
    f32x4* out = (f32x4*)(dst + (int64_t)b * total * 4);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int q = (int)(i % qz);
        const int64_t r = i / qz;
        const int j = (int)(r % py);
        const int a = (int)(r / py);
        const int sa = (flip & 1) ? px - 1 - a : a;
        const int sj = (flip & 2) ? py - 1 - j : j;
        const int sq = (flip & 4) ? qz - 1 - q : q;
        const f32x4 v = *(const f32x4*)(vol + ((int64_t)(ox + sa) * Y + (oy + sj)) * Z + oz + 4 * sq);
        f32x4 o;
        if (flip & 4) {
            o.x = v.w;
            o.y = v.z;
            o.z = v.y;
            o.w = v.x;
        } else {
            o = v;
        }
        out[i] = o;
    }
}

extern "C" int ru3d_predict_gather(const float* vol, int X, int Y, int Z, int cin, const int32_t* windows, int count,
                                   const ru3d_tensor* dst, void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    RU3D_REQUIRE(vol && windows && tensor_ok(dst), "predict_gather: bad argument");
    RU3D_REQUIRE(count >= 1 && count <= RU3D_PREDICT_MAX_BATCH, "predict_gather: %d windows in one launch (1..%d)",
                 count, RU3D_PREDICT_MAX_BATCH);
    RU3D_REQUIRE(dst->n == count, "predict_gather: %d windows for a batch of %d", count, dst->n);
    RU3D_REQUIRE(cin >= 1 && dst->c == cin && dst->ld == cin, "predict_gather: input must be dense with %d channels", cin);
    RU3D_REQUIRE(X > 0 && Y > 0 && Z > 0, "predict_gather: bad volume %dx%dx%d", X, Y, Z);
    GatherEntries e;
    bool aligned = true;
    for (int b = 0; b < RU3D_PREDICT_MAX_BATCH; b++) {
        const int s = b < count ? b : 0;
        e.ox[b] = windows[4 * s];
        e.oy[b] = windows[4 * s + 1];
        e.oz[b] = windows[4 * s + 2];
        e.flip[b] = windows[4 * s + 3];
        if (b >= count) continue;
        RU3D_REQUIRE(e.ox[b] >= 0 && e.oy[b] >= 0 && e.oz[b] >= 0 && e.ox[b] <= X - dst->d && e.oy[b] <= Y - dst->h &&
                         e.oz[b] <= Z - dst->w,
                     "predict_gather: window %d [%d+%d, %d+%d, %d+%d] outside the %dx%dx%d volume", b, e.ox[b], dst->d,
                     e.oy[b], dst->h, e.oz[b], dst->w, X, Y, Z);
        RU3D_REQUIRE(e.flip[b] >= 0 && e.flip[b] <= 7, "predict_gather: window %d has mirror mask %d (0..7)", b,
                     e.flip[b]);
        aligned = aligned && (e.oz[b] & 3) == 0;
    }
    hipStream_t st = as_stream(stream);
    const bool vec = cin == 1 && aligned && (dst->w & 3) == 0 && (Z & 3) == 0 && ((uintptr_t)vol & 15) == 0 &&
                     ((uintptr_t)dst->ptr & 15) == 0;
    const int64_t work = (int64_t)dst->d * dst->h * dst->w * cin / (vec ? 4 : 1);
    int blocks = (int)((work + 255) / 256);
    const int cap = (2048 + count - 1) / count;
    if (blocks > cap) blocks = cap;
    if (vec)
        hipLaunchKernelGGL(predict_gather_c1v4_kernel, dim3(blocks, count), dim3(256), 0, st, vol, Y, Z,
                           (float*)dst->ptr, dst->d, dst->h, dst->w, e);
    else
        hipLaunchKernelGGL(predict_gather_kernel, dim3(blocks, count), dim3(256), 0, st, vol, Y, Z, cin,
                           (float*)dst->ptr, dst->d, dst->h, dst->w, e);
    return ru3d_check_launch("predict_gather");
}

// ------------------------------------------------------------------------------------------------ accumulate
// the C logits of one voxel: one 4 / 8 / 16-byte load when the row is dense (ld == C) and C is 2 or 4
template <typename T, int C, bool VEC>
__device__ __forceinline__ void load_logits(const T* __restrict__ zp, float (&v)[C]) {
    if constexpr (VEC) {
        load_vec<T, C>(zp, v);
    } else {
#pragma unroll
        for (int c = 0; c < C; c++) v[c] = to_f32<T>(zp[c]);
    }
}

template <typename T, int C, bool VEC, bool WEIGHTED>
__global__ __launch_bounds__(256) void predict_accumulate_weighted_kernel(
    const T* __restrict__ z, int ld, int pd, int ph, int pw, int flip, const float* __restrict__ gx,
    const float* __restrict__ gy, const float* __restrict__ gz, float* __restrict__ acc, float* __restrict__ cnt, int Y,
    int Z, int ox, int oy, int oz) {
    const int64_t total = (int64_t)pd * ph * pw;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        // (a, j, k): the voxel inside the window on the VOLUME's grid; the model saw it at the mirrored index
        const int k = (int)(i % pw);
        const int64_t r = i / pw;
        const int j = (int)(r % ph);
        const int a = (int)(r / ph);
        const int sa = (flip & 1) ? pd - 1 - a : a;
        const int sj = (flip & 2) ? ph - 1 - j : j;
        const int sk = (flip & 4) ? pw - 1 - k : k;
        const T* zp = z + (((int64_t)sa * ph + sj) * pw + sk) * ld;
        float v[C];
        load_logits<T, C, VEC>(zp, v);
        float p[C];
        if (C == 1) {
            p[0] = 1.f / (1.f + __expf(-v[0]));                       // as predict_accumulate_kernel
        } else {
            float m = v[0];
#pragma unroll
            for (int c = 1; c < C; c++) m = fmaxf(m, v[c]);
            float se = 0.f;
#pragma unroll
            for (int c = 0; c < C; c++) {
                v[c] = expf(v[c] - m);
                se += v[c];
            }
#pragma unroll
            for (int c = 0; c < C; c++) p[c] = v[c] / se;
        }
        const int64_t o = ((int64_t)(ox + a) * Y + (oy + j)) * Z + (oz + k);
        float wgt = 1.f;
        if (WEIGHTED) {
            wgt = (gx[a] * gy[j]) * gz[k];
#pragma unroll
            for (int c = 0; c < C; c++) p[c] *= wgt;
        }
        float* ap = acc + o * C;
        if constexpr (C == 2 || C == 4) {                             // acc rows of 8 / 16 bytes are aligned
            float cur[C];
            load_vec<float, C>(ap, cur);
#pragma unroll
            for (int c = 0; c < C; c++) cur[c] += p[c];
            store_vec<float, C>(ap, cur);
        } else {
#pragma unroll
            for (int c = 0; c < C; c++) ap[c] += p[c];
        }
        cnt[o] += wgt;
    }
}

template <typename T, int C>
static void accumulate_weighted_pick(const T* z, const ru3d_tensor* t, int flip, const float* gx, const float* gy,
                                     const float* gz, float* acc, float* cnt, int Y, int Z, int ox, int oy, int oz,
                                     hipStream_t st) {
    const int64_t vox = (int64_t)t->d * t->h * t->w;
    int blocks = (int)((vox + 255) / 256);
    if (blocks > 2048) blocks = 2048;
    const bool vec = (C == 2 || C == 4) && t->ld == C && ((uintptr_t)z % (C * sizeof(T))) == 0;
#define RU3D_ACCW(VEC, WEIGHTED)                                                                                       \
    hipLaunchKernelGGL((predict_accumulate_weighted_kernel<T, C, VEC, WEIGHTED>), dim3(blocks), dim3(256), 0, st, z,   \
                       t->ld, t->d, t->h, t->w, flip, gx, gy, gz, acc, cnt, Y, Z, ox, oy, oz)
    if (gx) {
        if (vec) RU3D_ACCW(true, true);
        else RU3D_ACCW(false, true);
    } else {
        if (vec) RU3D_ACCW(true, false);
        else RU3D_ACCW(false, false);
    }
#undef RU3D_ACCW
}

template <int C>
static int accumulate_weighted_launch(const ru3d_tensor* t, int dtype, int sample, int flip, const float* gx,
                                      const float* gy, const float* gz, float* acc, float* cnt, int Y, int Z, int ox,
                                      int oy, int oz, hipStream_t st) {
    const int64_t off = (int64_t)sample * t->d * t->h * t->w * t->ld;
    if (dtype == RU3D_F32)
        accumulate_weighted_pick<float, C>((const float*)t->ptr + off, t, flip, gx, gy, gz, acc, cnt, Y, Z, ox, oy, oz,
                                           st);
    else
        accumulate_weighted_pick<bf16, C>((const bf16*)t->ptr + off, t, flip, gx, gy, gz, acc, cnt, Y, Z, ox, oy, oz,
                                          st);
    return ru3d_check_launch("predict_accumulate_weighted");
}

extern "C" int ru3d_predict_accumulate_weighted(const ru3d_tensor* logits, int dtype, int sample, int flip,
                                                const float* gx, const float* gy, const float* gz, float* acc,
                                                float* cnt, int X, int Y, int Z, int ox, int oy, int oz, void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    RU3D_REQUIRE(tensor_ok(logits) && acc && cnt, "predict_accumulate_weighted: bad argument");
    RU3D_REQUIRE(dtype == RU3D_F32 || dtype == RU3D_BF16, "predict_accumulate_weighted: dtype must be f32 or bf16");
    RU3D_REQUIRE(sample >= 0 && sample < logits->n, "predict_accumulate_weighted: sample %d outside batch of %d", sample,
                 logits->n);
    RU3D_REQUIRE(logits->c >= 1 && logits->c <= RU3D_PREDICT_MAX_CLASSES,
                 "predict_accumulate_weighted: %d classes (max %d)", logits->c, RU3D_PREDICT_MAX_CLASSES);
    RU3D_REQUIRE(flip >= 0 && flip <= 7, "predict_accumulate_weighted: mirror mask %d (0..7)", flip);
    RU3D_REQUIRE((gx && gy && gz) || (!gx && !gy && !gz),
                 "predict_accumulate_weighted: the three weight tables come together or not at all");
    RU3D_REQUIRE(ox >= 0 && oy >= 0 && oz >= 0 && ox <= X - logits->d && oy <= Y - logits->h && oz <= Z - logits->w,
                 "predict_accumulate_weighted: window [%d+%d, %d+%d, %d+%d] outside the %dx%dx%d volume", ox, logits->d,
                 oy, logits->h, oz, logits->w, X, Y, Z);
    hipStream_t st = as_stream(stream);
#define RU3D_ACCW_CASE(n) \
    case n: return accumulate_weighted_launch<n>(logits, dtype, sample, flip, gx, gy, gz, acc, cnt, Y, Z, ox, oy, oz, st)
    switch (logits->c) {
        RU3D_ACCW_CASE(1);
        RU3D_ACCW_CASE(2);
        RU3D_ACCW_CASE(3);
        RU3D_ACCW_CASE(4);
        RU3D_ACCW_CASE(5);
        RU3D_ACCW_CASE(6);
        RU3D_ACCW_CASE(7);
        default: return accumulate_weighted_launch<8>(logits, dtype, sample, flip, gx, gy, gz, acc, cnt, Y, Z, ox, oy, oz,
                                                      st);
    }
#undef RU3D_ACCW_CASE
}
