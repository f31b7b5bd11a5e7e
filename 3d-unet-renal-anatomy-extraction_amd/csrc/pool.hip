// 2x2x2 / stride-2 max pooling, forward and backward (MaxPoolBlock, reference network.py:452-463: nn.MaxPool3d(2, 2)).
//
// HBM-bound: forward reads x once and writes y (1/8 of x) and one code byte per element of y; backward reads dy and the
// codes and writes every element of dx once.  No LDS, no atomics, no arithmetic on the values: the output is a bit copy of
// the element that won, so ONE translation unit serves fp32, bf16 and fp16 (elements travel as integers; only the
// comparison looks at them as numbers).
//
// Work split: one lane owns one output voxel x one 16-byte channel group (8 channels of 16 bits, 4 of fp32); consecutive
// lanes take consecutive channel groups, then consecutive w, so the two dx taps of neighbouring output voxels are
// neighbours in memory and a wave consumes whole fetched lines.  All eight 16-byte loads are issued before the first
// compare.  Channel counts / pointers / pitches that do not allow 16-byte accesses take the element-per-lane kernels.
//
// The winner is torch's (aten max_pool3d_with_indices): scan the window in (d, h, w) order, replace the running maximum
// when v > max || isnan(v).  First of equal values wins, +0.0 against -0.0 keeps the first, every NaN replaces (the last
// NaN of a window wins).  The code is dz*4 + dy*2 + dx of the winner.
#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;

// KIND = the RU3D_* dtype code.  Bits: the element as an integer; VEC: elements per 16 bytes
template <int KIND> struct PoolElem;
template <> struct PoolElem<RU3D_F32> {
    typedef uint32_t Bits;
    static constexpr int VEC = 4;
    typedef uint32_t Codes;      // VEC code bytes
    static __device__ __forceinline__ float num(Bits b) { return __builtin_bit_cast(float, b); }
};
template <> struct PoolElem<RU3D_BF16> {
    typedef uint16_t Bits;
    static constexpr int VEC = 8;
    typedef uint2 Codes;
    static __device__ __forceinline__ float num(Bits b) { return __builtin_bit_cast(float, (uint32_t)b << 16); }
};
template <> struct PoolElem<RU3D_F16> {
    typedef uint16_t Bits;
    static constexpr int VEC = 8;
    typedef uint2 Codes;
    static __device__ __forceinline__ float num(Bits b) { return (float)__builtin_bit_cast(_Float16, b); }
};

struct PoolGeom {
    int D, H, W;          // extents of x / dx
    int OD, OH, OW;       // extents of y / dy: floor(D/2) ..
    int C;
    int64_t ldx, ldy;     // voxel pitches in elements
};

// torch's update rule
__device__ __forceinline__ bool pool_takes(float v, float m) { return v > m || v != v; }

// ------------------------------------------------------------------------------------------- forward, 16 bytes per lane
template <int KIND>
__global__ __launch_bounds__(256) void maxpool_fwd_vec_kernel(const typename PoolElem<KIND>::Bits* __restrict__ x,
                                                              typename PoolElem<KIND>::Bits* __restrict__ y,
                                                              uint8_t* __restrict__ idx, PoolGeom g, int64_t work) {
    typedef PoolElem<KIND> E;
    typedef typename E::Bits Bits;
    typedef __attribute__((ext_vector_type(E::VEC))) Bits BV;
    constexpr int VEC = E::VEC;
    const int G = g.C / VEC;
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < work; i += step) {
        const int64_t ov = i / G;
        const int cg = (int)(i - ov * G);
        int64_t r = ov / g.OW;
        const int ow = (int)(ov - r * g.OW);
        int64_t r2 = r / g.OH;
        const int oh = (int)(r - r2 * g.OH);
        const int64_t n = r2 / g.OD;
        const int od = (int)(r2 - n * g.OD);
        const int64_t vox0 = ((n * g.D + 2 * od) * g.H + 2 * oh) * g.W + 2 * ow;
        const Bits* base = x + vox0 * g.ldx + (int64_t)cg * VEC;
        BV t[8];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int64_t dv = ((int64_t)(k >> 2) * g.H + ((k >> 1) & 1)) * g.W + (k & 1);
            t[k] = __builtin_bit_cast(BV, *reinterpret_cast<const u32x4*>(base + dv * g.ldx));
        }
        BV out;
        uint8_t code[VEC];
#pragma unroll
        for (int j = 0; j < VEC; j++) {
            Bits mb = t[0][j];
            float m = E::num(mb);
            int c = 0;
#pragma unroll
            for (int k = 1; k < 8; k++) {
                const Bits vb = t[k][j];
                const float v = E::num(vb);
                const bool take = pool_takes(v, m);
                m = take ? v : m;
                mb = take ? vb : mb;
                c = take ? k : c;
            }
            out[j] = mb;
            code[j] = (uint8_t)c;
        }
        *reinterpret_cast<u32x4*>(y + ov * g.ldy + (int64_t)cg * VEC) = __builtin_bit_cast(u32x4, out);
        if (idx) {
            typename E::Codes packed;
            __builtin_memcpy(&packed, code, VEC);
            *reinterpret_cast<typename E::Codes*>(idx + ov * g.C + (int64_t)cg * VEC) = packed;
        }
    }
}

// ------------------------------------------------------------------------------------------- forward, one element per lane
template <int KIND>
__global__ __launch_bounds__(256) void maxpool_fwd_scalar_kernel(const typename PoolElem<KIND>::Bits* __restrict__ x,
                                                                 typename PoolElem<KIND>::Bits* __restrict__ y,
                                                                 uint8_t* __restrict__ idx, PoolGeom g, int64_t work) {
    typedef PoolElem<KIND> E;
    typedef typename E::Bits Bits;
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < work; i += step) {
        const int64_t ov = i / g.C;
        const int ch = (int)(i - ov * g.C);
        int64_t r = ov / g.OW;
        const int ow = (int)(ov - r * g.OW);
        int64_t r2 = r / g.OH;
        const int oh = (int)(r - r2 * g.OH);
        const int64_t n = r2 / g.OD;
        const int od = (int)(r2 - n * g.OD);
        const int64_t vox0 = ((n * g.D + 2 * od) * g.H + 2 * oh) * g.W + 2 * ow;
        const Bits* base = x + vox0 * g.ldx + ch;
        Bits t[8];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int64_t dv = ((int64_t)(k >> 2) * g.H + ((k >> 1) & 1)) * g.W + (k & 1);
            t[k] = base[dv * g.ldx];
        }
        Bits mb = t[0];
        float m = E::num(mb);
        int c = 0;
#pragma unroll
        for (int k = 1; k < 8; k++) {
            const float v = E::num(t[k]);
            const bool take = pool_takes(v, m);
            m = take ? v : m;
            mb = take ? t[k] : mb;
            c = take ? k : c;
        }
        y[ov * g.ldy + ch] = mb;
        if (idx) idx[ov * g.C + ch] = (uint8_t)c;
    }
}

// ------------------------------------------------------------------------------------------- backward
// The lanes walk the 2x2x2 CELLS of dx, ceil(D/2) x ceil(H/2) x ceil(W/2) of them: a cell inside the pooled extents is a
// window (dy goes to the tap its code names, zero to the other seven); a cell that hangs over an odd extent holds no
// window and its in-range voxels get zeros.  Every element of dx is written exactly once.
template <int KIND>
__global__ __launch_bounds__(256) void maxpool_bwd_vec_kernel(const typename PoolElem<KIND>::Bits* __restrict__ dy,
                                                              const uint8_t* __restrict__ idx,
                                                              typename PoolElem<KIND>::Bits* __restrict__ dx, PoolGeom g,
                                                              int CD, int CH, int CW, int64_t work) {
    typedef PoolElem<KIND> E;
    typedef typename E::Bits Bits;
    typedef __attribute__((ext_vector_type(E::VEC))) Bits BV;
    constexpr int VEC = E::VEC;
    const int G = g.C / VEC;
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < work; i += step) {
        const int64_t cell = i / G;
        const int cg = (int)(i - cell * G);
        int64_t r = cell / CW;
        const int ow = (int)(cell - r * CW);
        int64_t r2 = r / CH;
        const int oh = (int)(r - r2 * CH);
        const int64_t n = r2 / CD;
        const int od = (int)(r2 - n * CD);
        const bool window = od < g.OD && oh < g.OH && ow < g.OW;
        BV gy = (BV)(Bits)0;
        uint8_t code[VEC];
#pragma unroll
        for (int j = 0; j < VEC; j++) code[j] = 8;      // no tap
        if (window) {
            const int64_t ov = ((n * g.OD + od) * g.OH + oh) * g.OW + ow;
            gy = __builtin_bit_cast(BV, *reinterpret_cast<const u32x4*>(dy + ov * g.ldy + (int64_t)cg * VEC));
            typename E::Codes packed = *reinterpret_cast<const typename E::Codes*>(idx + ov * g.C + (int64_t)cg * VEC);
            __builtin_memcpy(code, &packed, VEC);
        }
        const int64_t vox0 = ((n * g.D + 2 * od) * g.H + 2 * oh) * g.W + 2 * ow;
        Bits* base = dx + vox0 * g.ldx + (int64_t)cg * VEC;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int dz = k >> 2, dyy = (k >> 1) & 1, dxx = k & 1;
            if (!window && (2 * od + dz >= g.D || 2 * oh + dyy >= g.H || 2 * ow + dxx >= g.W)) continue;
            BV o;
#pragma unroll
            for (int j = 0; j < VEC; j++) o[j] = code[j] == k ? gy[j] : (Bits)0;
            const int64_t dv = ((int64_t)dz * g.H + dyy) * g.W + dxx;
            *reinterpret_cast<u32x4*>(base + dv * g.ldx) = __builtin_bit_cast(u32x4, o);
        }
    }
}

template <int KIND>
__global__ __launch_bounds__(256) void maxpool_bwd_scalar_kernel(const typename PoolElem<KIND>::Bits* __restrict__ dy,
                                                                 const uint8_t* __restrict__ idx,
                                                                 typename PoolElem<KIND>::Bits* __restrict__ dx, PoolGeom g,
                                                                 int CD, int CH, int CW, int64_t work) {
    typedef typename PoolElem<KIND>::Bits Bits;
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < work; i += step) {
        const int64_t cell = i / g.C;
        const int ch = (int)(i - cell * g.C);
        int64_t r = cell / CW;
        const int ow = (int)(cell - r * CW);
        int64_t r2 = r / CH;
        const int oh = (int)(r - r2 * CH);
        const int64_t n = r2 / CD;
        const int od = (int)(r2 - n * CD);
        const bool window = od < g.OD && oh < g.OH && ow < g.OW;
        Bits gy = 0;
        int code = 8;
        if (window) {
            const int64_t ov = ((n * g.OD + od) * g.OH + oh) * g.OW + ow;
            gy = dy[ov * g.ldy + ch];
            code = idx[ov * g.C + ch];
        }
        const int64_t vox0 = ((n * g.D + 2 * od) * g.H + 2 * oh) * g.W + 2 * ow;
        Bits* base = dx + vox0 * g.ldx + ch;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int dz = k >> 2, dyy = (k >> 1) & 1, dxx = k & 1;
            if (!window && (2 * od + dz >= g.D || 2 * oh + dyy >= g.H || 2 * ow + dxx >= g.W)) continue;
            const int64_t dv = ((int64_t)dz * g.H + dyy) * g.W + dxx;
            base[dv * g.ldx] = code == k ? gy : (Bits)0;
        }
    }
}

// ------------------------------------------------------------------------------------------- host side
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// 16-byte accesses: the channel count is whole groups, and both tensors start and step on 16-byte boundaries
bool pool_vec_ok(const ru3d_tensor* full, const ru3d_tensor* pooled, const uint8_t* idx, int vec, int esize) {
    return full->c % vec == 0 && aligned16(full->ptr) && aligned16(pooled->ptr) && ((int64_t)full->ld * esize) % 16 == 0 &&
           ((int64_t)pooled->ld * esize) % 16 == 0 && ((uintptr_t)idx & 7) == 0;
}

unsigned pool_grid(int64_t work) {
    int64_t b = (work + 255) / 256;
    return (unsigned)(b < 1 ? 1 : (b > 2048 ? 2048 : b));
}

int pool_geometry(const char* what, const ru3d_tensor* full, const ru3d_tensor* pooled, int dtype, PoolGeom* g) {
    RU3D_REQUIRE(full && pooled && full->cseg == 0 && pooled->cseg == 0, "%s: split (planar) tensors are not accepted", what);
    RU3D_REQUIRE(dtype == RU3D_F32 || dtype == RU3D_BF16 || dtype == RU3D_F16, "%s: bad dtype %d", what, dtype);
    RU3D_REQUIRE(tensor_ok(full), "%s: bad full-resolution tensor", what);
    RU3D_REQUIRE(full->d >= 2 && full->h >= 2 && full->w >= 2, "%s: every spatial extent must be at least 2 (got %d x %d x %d)",
                 what, full->d, full->h, full->w);
    RU3D_REQUIRE(tensor_ok(pooled), "%s: bad pooled tensor", what);
    RU3D_REQUIRE(pooled->n == full->n && pooled->c == full->c && pooled->d == full->d / 2 && pooled->h == full->h / 2 &&
                     pooled->w == full->w / 2,
                 "%s: the pooled tensor must be [%d, %d, %d, %d, %d]", what, full->n, full->c, full->d / 2, full->h / 2,
                 full->w / 2);
    g->D = full->d, g->H = full->h, g->W = full->w;
    g->OD = pooled->d, g->OH = pooled->h, g->OW = pooled->w;
    g->C = full->c;
    g->ldx = full->ld, g->ldy = pooled->ld;
    return 0;
}

template <int KIND>
int maxpool_fwd_impl(const ru3d_tensor* x, const ru3d_tensor* y, uint8_t* idx, const PoolGeom& g, hipStream_t st) {
    typedef typename PoolElem<KIND>::Bits Bits;
    constexpr int VEC = PoolElem<KIND>::VEC;
    const int64_t outs = nvox(y);
    if (pool_vec_ok(x, y, idx, VEC, (int)sizeof(Bits))) {
        const int64_t work = outs * (g.C / VEC);
        hipLaunchKernelGGL(maxpool_fwd_vec_kernel<KIND>, dim3(pool_grid(work)), dim3(256), 0, st, (const Bits*)x->ptr,
                           (Bits*)y->ptr, idx, g, work);
    } else {
        const int64_t work = outs * g.C;
        hipLaunchKernelGGL(maxpool_fwd_scalar_kernel<KIND>, dim3(pool_grid(work)), dim3(256), 0, st, (const Bits*)x->ptr,
                           (Bits*)y->ptr, idx, g, work);
    }
    return ru3d_check_launch("maxpool3d_fwd");
}

template <int KIND>
int maxpool_bwd_impl(const ru3d_tensor* dy, const uint8_t* idx, const ru3d_tensor* dx, const PoolGeom& g, hipStream_t st) {
    typedef typename PoolElem<KIND>::Bits Bits;
    constexpr int VEC = PoolElem<KIND>::VEC;
    const int CD = (g.D + 1) / 2, CH = (g.H + 1) / 2, CW = (g.W + 1) / 2;
    const int64_t cells = (int64_t)dx->n * CD * CH * CW;
    if (pool_vec_ok(dx, dy, idx, VEC, (int)sizeof(Bits))) {
        const int64_t work = cells * (g.C / VEC);
        hipLaunchKernelGGL(maxpool_bwd_vec_kernel<KIND>, dim3(pool_grid(work)), dim3(256), 0, st, (const Bits*)dy->ptr, idx,
                           (Bits*)dx->ptr, g, CD, CH, CW, work);
    } else {
        const int64_t work = cells * g.C;
        hipLaunchKernelGGL(maxpool_bwd_scalar_kernel<KIND>, dim3(pool_grid(work)), dim3(256), 0, st, (const Bits*)dy->ptr,
                           idx, (Bits*)dx->ptr, g, CD, CH, CW, work);
    }
    return ru3d_check_launch("maxpool3d_bwd");
}

}  // namespace

extern "C" int ru3d_maxpool3d_fwd(const ru3d_tensor* x, const ru3d_tensor* y, uint8_t* idx, int dtype, void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    PoolGeom g;
    if (int rc = pool_geometry("maxpool3d_fwd", x, y, dtype, &g)) return rc;
    if (dtype == RU3D_F32) return maxpool_fwd_impl<RU3D_F32>(x, y, idx, g, as_stream(stream));
    if (dtype == RU3D_BF16) return maxpool_fwd_impl<RU3D_BF16>(x, y, idx, g, as_stream(stream));
    return maxpool_fwd_impl<RU3D_F16>(x, y, idx, g, as_stream(stream));
}

extern "C" int ru3d_maxpool3d_bwd(const ru3d_tensor* dy, const uint8_t* idx, const ru3d_tensor* dx, int dtype, void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    PoolGeom g;
    if (int rc = pool_geometry("maxpool3d_bwd", dx, dy, dtype, &g)) return rc;
    RU3D_REQUIRE(idx, "maxpool3d_bwd: the winner codes of the forward pass are required");
    if (dtype == RU3D_F32) return maxpool_bwd_impl<RU3D_F32>(dy, idx, dx, g, as_stream(stream));
    if (dtype == RU3D_BF16) return maxpool_bwd_impl<RU3D_BF16>(dy, idx, dx, g, as_stream(stream));
    return maxpool_bwd_impl<RU3D_F16>(dy, idx, dx, g, as_stream(stream));
}
