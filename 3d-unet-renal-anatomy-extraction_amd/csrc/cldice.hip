// Soft-clDice training loss (Shit et al., CVPR 2021): differentiable soft skeletons of float32 volumes, the loss sums,
// the on-device finalize and the whole backward down to dlogits.  Definition, tie rule and ABI: include/ru3d.h.
//
// One volume x[A][B][Z] (Z fastest) per (sample, class); `nvol` volumes lie behind one another ("planes" below are arrays
// of nvol * V floats).  With E the 7-point minimum and D the 27-point maximum, both clipped at the faces:
//   x_0 = x, x_{j+1} = E(x_j), d_j = relu(x_j - D(x_{j+1})), s_0 = d_0, s_j = s_{j-1} + relu(d_j - s_{j-1} d_j).
//
// Forward: erode_kernel writes x_{j+1} and the byte e_j[v] = which of the 7 candidates was the minimum; step_kernel
// reads x_j, the 27-window of x_{j+1} (LDS tile with halo) and s_{j-1}, writes d_j, s_j and the byte m_j[v] = which of
// the 27 candidates was the maximum.  The x chain lives in two scratch planes; d_j, s_j and the bytes are what the
// backward needs (it never looks at x again): relu' of d_j is [d_j > 0], and the extremal voxel is the saved byte.
//
// Backward: bwd_point_kernel walks j = k .. 0 in one thread per voxel (the s recurrence is pointwise) and writes
// h_j = dL/dd_j.  bwd_gather_kernel then forms, level by level from k + 1 down to 0,
//   gx_L[u] = h_L[u] - sum_{w in N27(u)} [argmax_w == u] h_{L-1}[w] + sum_{w in N7(u)} [argmin_w == u] gx_{L+1}[w]
// - the scatter of a window's gradient to its extremal voxel written as a gather over the windows that contain u, in a
// fixed order.  No atomics anywhere: two runs give the same bits.
#include "common.h"
#include "loss_core.h"
#include <stddef.h>

#define CD_MAX_ITER 64

// the tile of one workgroup (256 threads: thread = (b, z) column of the tile, looping over a) and its halo
constexpr int CD_TA = 8, CD_TB = 8, CD_TZ = 32;
constexpr int CD_HA = CD_TA + 2, CD_HB = CD_TB + 2, CD_HZ = CD_TZ + 2;
constexpr int CD_HALO = CD_HA * CD_HB * CD_HZ;

struct CdGeom {
    int A, B, Z;
    int nb, nz;        // tiles along B and Z
    int64_t tiles;     // tiles of one volume
    int64_t V;
};

struct CdState {
    double sums[5][RU3D_MAX_CLASSES];  // sum S(P) G, sum S(P), sum S(G) P, sum S(G), unused
    float w[RU3D_MAX_CLASSES];         // normalised class weights (slot order)
    float loss;
    int bad_labels;                    // at ru3d_loss_state_bad_labels_offset(): one read-back path for every loss
    float ca[RU3D_MAX_CLASSES];        // dL/dS(P)[v] = ca G[v] + cb
    float cb[RU3D_MAX_CLASSES];
    float cc[RU3D_MAX_CLASSES];        // dL/dP[v] (the plain P of Tsens) = cc S(G)[v]
};

extern "C" size_t ru3d_cldice_state_bytes(void) { return sizeof(CdState); }

static inline int64_t cd_ceil(int64_t a, int64_t b) { return (a + b - 1) / b; }

static CdGeom cd_geom(int A, int B, int Z) {
    CdGeom g;
    g.A = A;
    g.B = B;
    g.Z = Z;
    g.nb = (int)cd_ceil(B, CD_TB);
    g.nz = (int)cd_ceil(Z, CD_TZ);
    g.tiles = cd_ceil(A, CD_TA) * g.nb * g.nz;
    g.V = (int64_t)A * B * Z;
    return g;
}

static int cd_sum_blocks(int64_t total) {
    int64_t b = cd_ceil(total, 256 * 8);
    if (b > 1024) b = 1024;
    if (b < 1) b = 1;
    return (int)b;
}

static int cd_flat_blocks(int64_t total) { return flat_bwd_blocks(total, 16384); }

constexpr size_t CD_PART_BYTES = (size_t)1024 * 5 * RU3D_MAX_CLASSES * sizeof(double);

extern "C" size_t ru3d_cldice_workspace_bytes(int nvol, int A, int B, int Z, int iterations) {
    if (nvol <= 0 || A <= 0 || B <= 0 || Z <= 0 || iterations < 0) return 0;
    const int64_t plane = (int64_t)nvol * A * B * Z;
    // forward: P, G, two x planes, two s planes of the label chain; backward: k + 1 planes h, two planes gx
    const int64_t planes = (iterations + 3 > 6) ? iterations + 3 : 6;
    return CD_PART_BYTES + (size_t)(planes * plane) * sizeof(float);
}

// the workspace: the partial sums of the loss first (float64, the base is aligned), the planes behind them
static inline float* cd_planes(void* ws) { return (float*)((char*)ws + CD_PART_BYTES); }

// --------------------------------------------------------------------------- tiles
struct CdTile {
    int64_t base;   // element offset of the tile's volume inside a plane
    int a0, b0, z0;
};

__device__ __forceinline__ CdTile cd_tile(const CdGeom& g) {
    const int64_t blk = blockIdx.x;
    const int64_t vol = blk / g.tiles;
    int64_t r = blk - vol * g.tiles;
    CdTile t;
    t.z0 = (int)(r % g.nz) * CD_TZ;
    r /= g.nz;
    t.b0 = (int)(r % g.nb) * CD_TB;
    t.a0 = (int)(r / g.nb) * CD_TA;
    t.base = vol * g.V;
    return t;
}

// the tile with a one-voxel halo; whatever lies outside the volume reads as `fill`
template <typename T>
__device__ __forceinline__ void cd_load_halo(const T* __restrict__ vol, const CdGeom& g, const CdTile& t, T fill,
                                             T* __restrict__ tile) {
    for (int i = threadIdx.x; i < CD_HALO; i += 256) {
        const int hz = i % CD_HZ, hb = (i / CD_HZ) % CD_HB, ha = i / (CD_HZ * CD_HB);
        const int a = t.a0 + ha - 1, b = t.b0 + hb - 1, z = t.z0 + hz - 1;
        T v = fill;
        if (a >= 0 && a < g.A && b >= 0 && b < g.B && z >= 0 && z < g.Z) v = vol[((int64_t)a * g.B + b) * g.Z + z];
        tile[i] = v;
    }
}

#define CD_AT(tile, ha, hb, hz) tile[((ha) * CD_HB + (hb)) * CD_HZ + (hz)]

// --------------------------------------------------------------------------- forward chain
// y = E(x); emin[v] = index of the minimal candidate in the order (a-1), (b-1), (z-1), centre, (z+1), (b+1), (a+1):
// ascending linear index, strict comparison, so the first of equal minima wins
template <bool SAVE>
__global__ __launch_bounds__(256) void cd_erode_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                       uint8_t* __restrict__ emin, CdGeom g) {
    __shared__ float tile[CD_HALO];
    const CdTile t = cd_tile(g);
    cd_load_halo<float>(x + t.base, g, t, __builtin_inff(), tile);
    __syncthreads();
    const int tz = threadIdx.x & 31, tb = threadIdx.x >> 5;
    const int b = t.b0 + tb, z = t.z0 + tz;
    if (b >= g.B || z >= g.Z) return;
    for (int ta = 0; ta < CD_TA; ta++) {
        const int a = t.a0 + ta;
        if (a >= g.A) break;
        const int ha = ta + 1, hb = tb + 1, hz = tz + 1;
        const float c[7] = {CD_AT(tile, ha - 1, hb, hz), CD_AT(tile, ha, hb - 1, hz), CD_AT(tile, ha, hb, hz - 1),
                            CD_AT(tile, ha, hb, hz),     CD_AT(tile, ha, hb, hz + 1), CD_AT(tile, ha, hb + 1, hz),
                            CD_AT(tile, ha + 1, hb, hz)};
        float best = __builtin_inff();
        int bi = 3;
#pragma unroll
        for (int i = 0; i < 7; i++)
            if (c[i] < best) {
                best = c[i];
                bi = i;
            }
        const int64_t o = t.base + ((int64_t)a * g.B + b) * g.Z + z;
        y[o] = (bi == 3) ? c[3] : best;
        if (SAVE) emin[o] = (uint8_t)bi;
    }
}

// d_j = relu(x_j - D(x_{j+1})), s_j = s_{j-1} + relu(d_j - s_{j-1} d_j)  (s_0 = d_0: sprev == nullptr);
// dmax[v] = index of the maximal candidate among the 27 offsets in ascending (da, db, dz)
template <bool SAVE>
__global__ __launch_bounds__(256) void cd_step_kernel(const float* __restrict__ xj, const float* __restrict__ xj1,
                                                      const float* __restrict__ sprev, float* __restrict__ sout,
                                                      float* __restrict__ delta, uint8_t* __restrict__ dmax, CdGeom g) {
#pragma clang fp contract(off)   // d - s * d as the definition writes it, not as one fused operation
    __shared__ float tile[CD_HALO];
    const CdTile t = cd_tile(g);
    cd_load_halo<float>(xj1 + t.base, g, t, -__builtin_inff(), tile);
    __syncthreads();
    const int tz = threadIdx.x & 31, tb = threadIdx.x >> 5;
    const int b = t.b0 + tb, z = t.z0 + tz;
    if (b >= g.B || z >= g.Z) return;
    for (int ta = 0; ta < CD_TA; ta++) {
        const int a = t.a0 + ta;
        if (a >= g.A) break;
        float best = -__builtin_inff();
        int bi = 13;
#pragma unroll
        for (int i = 0; i < 27; i++) {
            const float c = CD_AT(tile, ta + i / 9, tb + (i / 3) % 3, tz + i % 3);
            if (c > best) {
                best = c;
                bi = i;
            }
        }
        if (bi == 13) best = CD_AT(tile, ta + 1, tb + 1, tz + 1);
        const int64_t o = t.base + ((int64_t)a * g.B + b) * g.Z + z;
        const float d = fmaxf(xj[o] - best, 0.f);
        float s = d;
        if (sprev) {
            const float sp = sprev[o];
            s = sp + fmaxf(d - sp * d, 0.f);
        }
        sout[o] = s;
        if (SAVE) {
            delta[o] = d;
            dmax[o] = (uint8_t)bi;
        }
    }
}

// the chain on `x0` (nvol volumes).  SAVE: d_j, s_j, e_j, m_j go to plane j of delta / s / emin / dmax (k + 1 planes
// each) and the result is plane k of s.  Otherwise s_j alternates between the two planes of `s` and s_k goes to `out`.
static int cd_chain(const float* x0, float* xa, float* xb, int nvol, const CdGeom& g, int k, bool save, float* delta,
                    float* s, uint8_t* emin, uint8_t* dmax, float* out, hipStream_t st) {
    const int64_t plane = (int64_t)nvol * g.V;
    const unsigned blocks = (unsigned)(g.tiles * nvol);
    const float* xj = x0;
    float* nxt = xa;
    const float* sprev = nullptr;
    for (int j = 0; j <= k; j++) {
        float* xj1 = nxt;
        float* sj;
        if (save) {
            hipLaunchKernelGGL(cd_erode_kernel<true>, dim3(blocks), dim3(256), 0, st, xj, xj1, emin + j * plane, g);
            sj = s + j * plane;
        } else {
            hipLaunchKernelGGL(cd_erode_kernel<false>, dim3(blocks), dim3(256), 0, st, xj, xj1, (uint8_t*)nullptr, g);
            sj = (j == k) ? out : s + (j & 1) * plane;
        }
        int rc = ru3d_check_launch("cldice_erode");
        if (rc) return rc;
        if (save)
            hipLaunchKernelGGL(cd_step_kernel<true>, dim3(blocks), dim3(256), 0, st, xj, (const float*)xj1, sprev, sj,
                               delta + j * plane, dmax + j * plane, g);
        else
            hipLaunchKernelGGL(cd_step_kernel<false>, dim3(blocks), dim3(256), 0, st, xj, (const float*)xj1, sprev, sj,
                               (float*)nullptr, (uint8_t*)nullptr, g);
        rc = ru3d_check_launch("cldice_step");
        if (rc) return rc;
        sprev = sj;
        xj = xj1;
        nxt = (xj1 == xa) ? xb : xa;
    }
    return 0;
}

// --------------------------------------------------------------------------- backward chain
// h_j = dL/dd_j for j = k .. 0 from gs = dL/ds_k.  gs comes from `gout` (a plane) or, for the loss, from the state
// block: gs[v] = ca G[v] + cb with G read from the labels.
__global__ __launch_bounds__(256) void cd_bwd_point_kernel(const float* __restrict__ gout,
                                                           const void* __restrict__ labels, int label_dtype,
                                                           ClassList cl, const CdState* __restrict__ st,
                                                           const float* __restrict__ delta, const float* __restrict__ s,
                                                           float* __restrict__ h, int64_t V, int64_t plane, int k) {
#pragma clang fp contract(off)
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < plane; i += (int64_t)gridDim.x * 256) {
        float gs;
        if (gout) {
            gs = gout[i];
        } else {
            const int64_t vol = i / V, v = i - vol * V;
            const int slot = (int)(vol % cl.K);
            const int64_t n = vol / cl.K;
            int c = cl.cls[0];
#pragma unroll
            for (int q = 1; q < RU3D_MAX_CLASSES; q++)
                if (q == slot) c = cl.cls[q];
            const int64_t li = n * V + v;
            const int t = (label_dtype == RU3D_LABEL_I64) ? (int)((const int64_t*)labels)[li]
                                                          : (int)((const uint8_t*)labels)[li];
            gs = (t == c ? st->ca[slot] : 0.f) + st->cb[slot];
        }
        for (int j = k; j >= 1; j--) {
            const float d = delta[j * plane + i], sp = s[(j - 1) * plane + i];
            const bool m = (d - sp * d) > 0.f;
            h[j * plane + i] = m ? gs * (1.f - sp) : 0.f;
            if (m) gs = gs - gs * d;
        }
        h[i] = delta[i] > 0.f ? gs : 0.f;
    }
}

// gx_L = h_L - D^T(h_{L-1}) + E^T(gx_{L+1}); a null pointer drops its term (h_L at L = k + 1, h_{L-1} at L = 0,
// gx_{L+1} at L = k + 1).  Window w = u + offset i holds u at offset (26 - i) resp. (6 - i).
__global__ __launch_bounds__(256) void cd_bwd_gather_kernel(const float* __restrict__ hl, const float* __restrict__ hm,
                                                            const uint8_t* __restrict__ dmax,
                                                            const float* __restrict__ gxn,
                                                            const uint8_t* __restrict__ emin, float* __restrict__ gx,
                                                            CdGeom g) {
    __shared__ float th[CD_HALO];
    __shared__ uint8_t tm[CD_HALO];
    const CdTile t = cd_tile(g);
    if (hm) {
        cd_load_halo<float>(hm + t.base, g, t, 0.f, th);
        cd_load_halo<uint8_t>(dmax + t.base, g, t, (uint8_t)255, tm);   // 255: no window there
    }
    __syncthreads();
    const int tz = threadIdx.x & 31, tb = threadIdx.x >> 5;
    const int b = t.b0 + tb, z = t.z0 + tz;
    if (b >= g.B || z >= g.Z) return;
    const int64_t sb = g.Z, sa = (int64_t)g.B * g.Z;
    for (int ta = 0; ta < CD_TA; ta++) {
        const int a = t.a0 + ta;
        if (a >= g.A) break;
        const int64_t o = t.base + (int64_t)a * sa + (int64_t)b * sb + z;
        float acc = hl ? hl[o] : 0.f;
        if (hm) {
            float sub = 0.f;
#pragma unroll
            for (int i = 0; i < 27; i++) {
                const int q = ((ta + i / 9) * CD_HB + tb + (i / 3) % 3) * CD_HZ + tz + i % 3;
                if (tm[q] == 26 - i) sub += th[q];
            }
            acc -= sub;
        }
        if (gxn) {
            float add = 0.f;
            if (a > 0 && emin[o - sa] == 6) add += gxn[o - sa];
            if (b > 0 && emin[o - sb] == 5) add += gxn[o - sb];
            if (z > 0 && emin[o - 1] == 4) add += gxn[o - 1];
            if (emin[o] == 3) add += gxn[o];
            if (z + 1 < g.Z && emin[o + 1] == 2) add += gxn[o + 1];
            if (b + 1 < g.B && emin[o + sb] == 1) add += gxn[o + sb];
            if (a + 1 < g.A && emin[o + sa] == 0) add += gxn[o + sa];
            acc += add;
        }
        gx[o] = acc;
    }
}

// gx_0 into `gx_out`; ws: k + 1 planes h, then two planes gx
static int cd_chain_bwd(const float* gout, const void* labels, int label_dtype, const ClassList& cl, const CdState* state,
                        int nvol, const CdGeom& g, int k, const float* delta, const float* s, const uint8_t* emin,
                        const uint8_t* dmax, float* gx_out, float* ws, hipStream_t st) {
    const int64_t plane = (int64_t)nvol * g.V;
    float* h = ws;
    float* ga = ws + (int64_t)(k + 1) * plane;
    float* gb = ga + plane;
    hipLaunchKernelGGL(cd_bwd_point_kernel, dim3(cd_flat_blocks(plane)), dim3(256), 0, st, gout, labels, label_dtype, cl,
                       state, delta, s, h, g.V, plane, k);
    int rc = ru3d_check_launch("cldice_bwd_point");
    if (rc) return rc;
    const unsigned blocks = (unsigned)(g.tiles * nvol);
    const float* gxn = nullptr;
    for (int L = k + 1; L >= 0; L--) {
        float* dst = (L == 0) ? gx_out : ((L & 1) ? ga : gb);
        hipLaunchKernelGGL(cd_bwd_gather_kernel, dim3(blocks), dim3(256), 0, st,
                           L <= k ? (const float*)(h + (int64_t)L * plane) : (const float*)nullptr,
                           L >= 1 ? (const float*)(h + (int64_t)(L - 1) * plane) : (const float*)nullptr,
                           L >= 1 ? dmax + (int64_t)(L - 1) * plane : (const uint8_t*)nullptr, gxn,
                           L <= k ? emin + (int64_t)L * plane : (const uint8_t*)nullptr, dst, g);
        rc = ru3d_check_launch("cldice_bwd_gather");
        if (rc) return rc;
        gxn = dst;
    }
    return 0;
}

static int cd_check_geom(const char* what, int nvol, int A, int B, int Z, int iterations) {
    RU3D_REQUIRE(nvol > 0 && A > 0 && B > 0 && Z > 0, "%s: empty volume", what);
    RU3D_REQUIRE(iterations >= 0 && iterations <= CD_MAX_ITER, "%s: iterations = %d (0 .. %d)", what, iterations,
                 CD_MAX_ITER);
    RU3D_REQUIRE((int64_t)A * B * Z < ((int64_t)1 << 31), "%s: a volume of 2^31 voxels or more", what);
    const CdGeom g = cd_geom(A, B, Z);
    RU3D_REQUIRE(g.tiles * nvol < ((int64_t)1 << 31), "%s: too many tiles for one launch", what);
    return 0;
}

extern "C" int ru3d_soft_skeleton_fwd(const float* x, int nvol, int A, int B, int Z, int iterations, float* delta,
                                      float* s, uint8_t* emin, uint8_t* dmax, void* ws, size_t ws_bytes, void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    RU3D_REQUIRE(x && delta && s && emin && dmax && ws, "soft_skeleton_fwd: null pointer");
    int rc = cd_check_geom("soft_skeleton_fwd", nvol, A, B, Z, iterations);
    if (rc) return rc;
    RU3D_REQUIRE(ws_bytes >= ru3d_cldice_workspace_bytes(nvol, A, B, Z, iterations),
                 "soft_skeleton_fwd: workspace too small");
    const CdGeom g = cd_geom(A, B, Z);
    float* xa = cd_planes(ws);
    return cd_chain(x, xa, xa + (int64_t)nvol * g.V, nvol, g, iterations, true, delta, s, emin, dmax, nullptr,
                    as_stream(stream));
}

extern "C" int ru3d_soft_skeleton_bwd(const float* grad_out, int nvol, int A, int B, int Z, int iterations,
                                      const float* delta, const float* s, const uint8_t* emin, const uint8_t* dmax,
                                      float* grad_x, void* ws, size_t ws_bytes, void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    RU3D_REQUIRE(grad_out && delta && s && emin && dmax && grad_x && ws, "soft_skeleton_bwd: null pointer");
    int rc = cd_check_geom("soft_skeleton_bwd", nvol, A, B, Z, iterations);
    if (rc) return rc;
    RU3D_REQUIRE(ws_bytes >= ru3d_cldice_workspace_bytes(nvol, A, B, Z, iterations),
                 "soft_skeleton_bwd: workspace too small");
    ClassList cl = {};
    cl.K = 1;
    return cd_chain_bwd(grad_out, nullptr, 0, cl, nullptr, nvol, cd_geom(A, B, Z), iterations, delta, s, emin, dmax,
                        grad_x, cd_planes(ws), as_stream(stream));
}

// --------------------------------------------------------------------------- the loss

// P and G planes [n][slot][v] of the selected classes
template <int C>
__global__ __launch_bounds__(256) void cd_softmax_kernel(const float* __restrict__ logits, int64_t stride_n,
                                                         int64_t stride_c, int64_t stride_v,
                                                         const void* __restrict__ labels, int label_dtype, int n,
                                                         int64_t V, ClassList cl, float* __restrict__ P,
                                                         float* __restrict__ G) {
    const int64_t total = (int64_t)n * V;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t ni = i / V, vi = i - ni * V;
        float p[C];
        softmax_probs<C>(logits + ni * stride_n + vi * stride_v, stride_c, p);
        const int t = load_label(labels, label_dtype, i);
#pragma unroll
        for (int c = 0; c < C; c++) {
            const int slot = cl.slot[c];
            if (slot >= 0) {
                const int64_t o = (ni * cl.K + slot) * V + vi;
                P[o] = p[c];
                G[o] = (t == c) ? 1.f : 0.f;
            }
        }
    }
}

// blockIdx.y = slot; partials part[block][slot * 5 + q], q = sum S(P) G, sum S(P), sum S(G) P, sum S(G), bad labels
__global__ __launch_bounds__(256) void cd_sums_kernel(const float* __restrict__ SP, const float* __restrict__ SG,
                                                      const float* __restrict__ P, const void* __restrict__ labels,
                                                      int label_dtype, int n, int64_t V, int C, ClassList cl,
                                                      double* __restrict__ part) {
    const int slot = blockIdx.y;
    int c = cl.cls[0];
#pragma unroll
    for (int q = 1; q < RU3D_MAX_CLASSES; q++)
        if (q == slot) c = cl.cls[q];
    float acc[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    const int64_t total = (int64_t)n * V;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t ni = i / V, vi = i - ni * V;
        const int64_t o = (ni * cl.K + slot) * V + vi;
        const int t = load_label(labels, label_dtype, i);
        const float sp = SP[o], sg = SG[o];
        if (t == c) acc[0] += sp;
        acc[1] += sp;
        acc[2] = fmaf(sg, P[o], acc[2]);
        acc[3] += sg;
        if (t < 0 || t >= C) acc[4] += 1.f;
    }
    __shared__ double sh[4][5];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < 5; q++) {
        const float r = wave_sum(acc[q]);
        if (lane == 0) sh[wid][q] = r;
    }
    __syncthreads();
    if (threadIdx.x < 5) {
        const int q = threadIdx.x;
        part[(int64_t)blockIdx.x * (5 * cl.K) + slot * 5 + q] = (sh[0][q] + sh[1][q]) + (sh[2][q] + sh[3][q]);
    }
}

struct CdParams {
    int K;
    float smooth;
    float w[RU3D_MAX_CLASSES];   // weight_v of the selected classes, un-normalised
};

// one workgroup: thread (g, q) adds the partials of quantity q over the blocks g, g + NG, ..; the NG group sums are then
// added in group order (region_reduce_rows of loss_core.h)
constexpr int CD_FIN_THREADS = 1024;
__global__ __launch_bounds__(CD_FIN_THREADS) void cd_finalize_kernel(const double* __restrict__ part, int blocks,
                                                                     CdParams P, CdState* __restrict__ st,
                                                                     float* __restrict__ loss_out) {
    constexpr int QMAX = 5 * RU3D_MAX_CLASSES;
    __shared__ double red[CD_FIN_THREADS];
    __shared__ double tot[QMAX];
    const int Q = 5 * P.K, NG = CD_FIN_THREADS / Q;
    const int gi = threadIdx.x / Q, q = threadIdx.x % Q;
    if (gi < NG) {
        double s0 = 0.0;
        for (int b = gi; b < blocks; b += NG) s0 += part[(int64_t)b * Q + q];
        red[gi * Q + q] = s0;
    }
    __syncthreads();
    if (threadIdx.x < Q) {
        double t = 0.0;
        for (int k = 0; k < NG; k++) t += red[k * Q + threadIdx.x];
        tot[threadIdx.x] = t;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double wsum = 0.0;
    for (int k = 0; k < P.K; k++) wsum += fabs((double)P.w[k]);
    if (wsum < 1e-12) wsum = 1e-12;
    const double eps = P.smooth;
    double loss = 0.0;
    for (int k = 0; k < RU3D_MAX_CLASSES; k++) {
        st->w[k] = st->ca[k] = st->cb[k] = st->cc[k] = 0.f;
        for (int q5 = 0; q5 < 5; q5++) st->sums[q5][k] = (k < P.K) ? tot[k * 5 + q5] : 0.0;
    }
    for (int k = 0; k < P.K; k++) {
        const double w = (double)P.w[k] / wsum;
        const double tp = tot[k * 5 + 0], a = tot[k * 5 + 1], ts = tot[k * 5 + 2], b = tot[k * 5 + 3];
        const double Tp = (tp + eps) / (a + eps), Ts = (ts + eps) / (b + eps);
        const double cld = 2.0 * Tp * Ts / (Tp + Ts);
        loss += w * (1.0 - cld);
        const double dTp = 2.0 * Ts * Ts / ((Tp + Ts) * (Tp + Ts)), dTs = 2.0 * Tp * Tp / ((Tp + Ts) * (Tp + Ts));
        st->w[k] = (float)w;
        st->ca[k] = (float)(-w * dTp / (a + eps));
        st->cb[k] = (float)(w * dTp * (tp + eps) / ((a + eps) * (a + eps)));
        st->cc[k] = (float)(-w * dTs / (b + eps));
    }
    st->bad_labels = (int)tot[4];
    if (st->bad_labels > 0) loss = nan("");   // F.one_hot would have raised
    st->loss = (float)loss;
    loss_out[0] = (float)loss;
}

// dlogits (+)= grad_out[0] * scale * softmax'(dP), dP_c = gx0_c + cc_c S(G_c) for the selected classes, 0 otherwise
template <int C, bool ACC>
__global__ __launch_bounds__(256) void cd_logits_bwd_kernel(const float* __restrict__ logits, int64_t stride_n,
                                                            int64_t stride_c, int64_t stride_v, int n, int64_t V,
                                                            ClassList cl, const CdState* __restrict__ st,
                                                            const float* __restrict__ gx0, const float* __restrict__ SG,
                                                            const float* __restrict__ grad_out, float scale,
                                                            float* __restrict__ dz) {
    const float go = (grad_out ? grad_out[0] : 1.f) * scale;
    float cc[C];
#pragma unroll
    for (int c = 0; c < C; c++) {
        cc[c] = 0.f;
#pragma unroll
        for (int q = 0; q < RU3D_MAX_CLASSES; q++)
            if (cl.slot[c] == q) cc[c] = st->cc[q];
    }
    const int64_t total = (int64_t)n * V;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t ni = i / V, vi = i - ni * V;
        const int64_t base = ni * stride_n + vi * stride_v;
        float p[C], u[C];
        softmax_probs<C>(logits + base, stride_c, p);
        float su = 0.f;
#pragma unroll
        for (int c = 0; c < C; c++) {
            const int slot = cl.slot[c];
            float dp = 0.f;
            if (slot >= 0) {
                const int64_t o = (ni * cl.K + slot) * V + vi;
                dp = gx0[o] + cc[c] * SG[o];
            }
            u[c] = p[c] * dp;
            su += u[c];
        }
#pragma unroll
        for (int c = 0; c < C; c++) {
            const float d = (u[c] - p[c] * su) * go;
            if (ACC)
                dz[base + c * stride_c] += d;
            else
                dz[base + c * stride_c] = d;
        }
    }
}

extern "C" int ru3d_cldice_fwd(const float* logits, int64_t stride_n, int64_t stride_c, int64_t stride_v,
                               const void* labels, int label_dtype, int n, int A, int B, int Z, int num_classes,
                               const int* classes, int num_selected, int iterations, const float* weight_v, float smooth,
                               float* delta, float* s, uint8_t* emin, uint8_t* dmax, float* skel_g, void* state,
                               float* loss_out, void* ws, size_t ws_bytes, void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    int rc = loss_view_check("cldice_fwd",
                             logits && labels && delta && s && emin && dmax && skel_g && state && loss_out && ws,
                             n > 0 && A > 0 && B > 0 && Z > 0, label_dtype, num_classes, 2);
    if (rc) return rc;
    RU3D_REQUIRE(offsetof(CdState, bad_labels) == ru3d_loss_state_bad_labels_offset(),
                 "cldice_fwd: state layouts out of step");
    ClassList cl;
    rc = class_list_check("cldice_fwd", num_classes, classes, num_selected, &cl);
    if (rc) return rc;
    RU3D_REQUIRE((int64_t)n * cl.K < ((int64_t)1 << 31), "cldice_fwd: bad batch");
    const int nvol = n * cl.K;
    rc = cd_check_geom("cldice_fwd", nvol, A, B, Z, iterations);
    if (rc) return rc;
    RU3D_REQUIRE(ws_bytes >= ru3d_cldice_workspace_bytes(nvol, A, B, Z, iterations), "cldice_fwd: workspace too small");
    hipStream_t st = as_stream(stream);
    const CdGeom g = cd_geom(A, B, Z);
    const int64_t plane = (int64_t)nvol * g.V, total = (int64_t)n * g.V;
    float* P = cd_planes(ws);
    float* G = P + plane;
    float* xa = G + plane;
    float* xb = xa + plane;
    float* sg2 = xb + plane;   // two planes
    double* part = (double*)ws;
#define CALL(CC)                                                                                                 \
    hipLaunchKernelGGL(cd_softmax_kernel<CC>, dim3(cd_flat_blocks(total)), dim3(256), 0, st, logits, stride_n, \
                       stride_c, stride_v, labels, label_dtype, n, g.V, cl, P, G)
    RU3D_DISPATCH_C(2, num_classes, CALL)
#undef CALL
    rc = ru3d_check_launch("cldice_softmax");
    if (rc) return rc;
    rc = cd_chain(P, xa, xb, nvol, g, iterations, true, delta, s, emin, dmax, nullptr, st);
    if (rc) return rc;
    rc = cd_chain(G, xa, xb, nvol, g, iterations, false, nullptr, sg2, nullptr, nullptr, skel_g, st);
    if (rc) return rc;
    const int blocks = cd_sum_blocks(total);
    hipLaunchKernelGGL(cd_sums_kernel, dim3(blocks, cl.K), dim3(256), 0, st,
                       (const float*)(s + (int64_t)iterations * plane), (const float*)skel_g, (const float*)P, labels,
                       label_dtype, n, g.V, num_classes, cl, part);
    rc = ru3d_check_launch("cldice_sums");
    if (rc) return rc;
    CdParams Pm;
    Pm.K = cl.K;
    Pm.smooth = smooth;
    fill_class_weights(Pm.w, weight_v, cl.K, cl.cls);
    hipLaunchKernelGGL(cd_finalize_kernel, dim3(1), dim3(CD_FIN_THREADS), 0, st, (const double*)part, blocks, Pm,
                       (CdState*)state, loss_out);
    return ru3d_check_launch("cldice_finalize");
}

extern "C" int ru3d_cldice_bwd(const float* logits, int64_t stride_n, int64_t stride_c, int64_t stride_v,
                               const void* labels, int label_dtype, int n, int A, int B, int Z, int num_classes,
                               const int* classes, int num_selected, int iterations, const float* delta, const float* s,
                               const uint8_t* emin, const uint8_t* dmax, const float* skel_g, const void* state,
                               const float* grad_out, float scale, int accumulate, float* dlogits, void* ws,
                               size_t ws_bytes, void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    int rc = loss_view_check("cldice_bwd",
                             logits && labels && delta && s && emin && dmax && skel_g && state && dlogits && ws,
                             n > 0 && A > 0 && B > 0 && Z > 0, label_dtype, num_classes, 2);
    if (rc) return rc;
    ClassList cl;
    rc = class_list_check("cldice_bwd", num_classes, classes, num_selected, &cl);
    if (rc) return rc;
    RU3D_REQUIRE((int64_t)n * cl.K < ((int64_t)1 << 31), "cldice_bwd: bad batch");
    const int nvol = n * cl.K;
    rc = cd_check_geom("cldice_bwd", nvol, A, B, Z, iterations);
    if (rc) return rc;
    RU3D_REQUIRE(ws_bytes >= ru3d_cldice_workspace_bytes(nvol, A, B, Z, iterations), "cldice_bwd: workspace too small");
    hipStream_t st = as_stream(stream);
    const CdGeom g = cd_geom(A, B, Z);
    const int64_t plane = (int64_t)nvol * g.V, total = (int64_t)n * g.V;
    // gx_0 goes into the chain's even gx plane: level 1, the last one to write scratch, wrote the odd one
    float* gx0 = cd_planes(ws) + (int64_t)(iterations + 2) * plane;
    rc = cd_chain_bwd(nullptr, labels, label_dtype, cl, (const CdState*)state, nvol, g, iterations, delta, s, emin, dmax,
                      gx0, cd_planes(ws), st);
    if (rc) return rc;
#define CALL(CC)                                                                                                       \
    if (accumulate)                                                                                                    \
        hipLaunchKernelGGL((cd_logits_bwd_kernel<CC, true>), dim3(cd_flat_blocks(total)), dim3(256), 0, st, logits,    \
                           stride_n, stride_c, stride_v, n, g.V, cl, (const CdState*)state, (const float*)gx0, skel_g, \
                           grad_out, scale, dlogits);                                                                  \
    else                                                                                                               \
        hipLaunchKernelGGL((cd_logits_bwd_kernel<CC, false>), dim3(cd_flat_blocks(total)), dim3(256), 0, st, logits,   \
                           stride_n, stride_c, stride_v, n, g.V, cl, (const CdState*)state, (const float*)gx0, skel_g, \
                           grad_out, scale, dlogits)
    RU3D_DISPATCH_C(2, num_classes, CALL)
#undef CALL
    return ru3d_check_launch("cldice_logits_bwd");
}
