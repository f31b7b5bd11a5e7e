// Boundary loss (Kervadec et al., MIDL 2019): the signed distance maps of a label patch - per sample and per selected
// class, all of them in one launch sequence - and the fused softmax x distance loss with its backward down to dlogits.
// Definition, degenerate rule and ABI: include/ru3d.h.
//
// One volume [A][B][Z] (Z fastest) per (sample, slot); volume (n, slot) has the index n * K + slot and its foreground is
// G = {label == classes[slot]}.  Every voxel needs the squared distance to the nearest voxel of the OTHER kind only, so
// one int32 per voxel carries both transforms through all three passes: s[v] > 0 is a background voxel's squared
// distance to the foreground found so far, s[v] < 0 minus a foreground voxel's squared distance to the background,
// +-BD_BIG where nothing of the other kind has been met yet.  A candidate l' of the other kind costs 0, one of the own
// kind costs |s[l']| - which is what that voxel knows about the kind this one looks for.  Everything is an integer:
// d^2 <= 3 (RU3D_BOUNDARY_MAX_AXIS - 1)^2 < 2^24, and BD_BIG + (L - 1)^2 stays below 2^31.
//   bd_pack_kernel     one read of the labels for all K slots: a wave takes 64 voxels of a Z row a trip, one ballot per
//                      slot gives the packed word (bit z - 64 w of bits[vol][a][b][w], zero at z >= Z).  Sets, per volume,
//                      the flag bits 1 (a foreground voxel) and 2 (a background voxel) with an integer atomicOr - gathered
//                      in registers, one per wave, sample and slot at most - and counts the labels outside [0, C) with an
//                      integer atomicAdd.  A volume whose flag is not 3 is degenerate:
//                      its maps are zero and the two scan kernels skip it.
//   bd_zy_kernel       Z and B passes of one a-plane and one tile of T columns of z.  Z pass: the nearest bit of the
//                      other kind below and above z, by bitvol.h's walk over the packed row XOR the voxel's own
//                      kind.  The [B][T] tile of s lives in LDS; every output scans outward d = 1, 2, .. on both
//                      sides and stops once d^2 alone reaches the best so far; hard bound d <= max(b, B - 1 - b).
//   bd_x_kernel        the same scan along A over an [A][T] tile staged in LDS, then the result: the signed square and
//                      phi = +sqrt(d2) outside, -(sqrt(d2) - 1) inside, the square root correctly rounded.
//                      A polarity for which the tile holds no information at all is not scanned.
//   bd_loss_kernel / bd_finalize_kernel / bd_bwd_kernel   sum_q w_q P_q phi_q in float64 partials over a partition fixed
//                      by the shape (2048 voxels a block, at most 1024 blocks) and a fixed tree; no floating-point
//                      atomics anywhere: the same bits in every run and under every CU budget.
#include <math.h>
#include <stddef.h>
#include "common.h"
#include "bitvol.h"
#include "loss_core.h"

#pragma clang fp contract(off)

typedef unsigned long long bd_u64;

#define BD_THREADS 512                    // workgroup of the two scan kernels
#define BD_TILE 8192                      // int32 of one LDS tile: 32 KiB, four workgroups a CU and room to spare
#define BD_MAX_COLS 32                    // columns of z per tile at most: 128-byte segments of the int32 plane
#define BD_BIG (1 << 30)                  // "nothing of the other kind met yet"
#define BD_PART 1024                      // partial sums of the loss at most = threads of the finalize
#define BD_PER_BLOCK 2048                 // voxels per partial at least

struct BdState {
    double total;                      // sum_q w_q sum P_q phi_q
    double pad0[31];
    float w[RU3D_MAX_CLASSES];         // normalised class weights (slot order)
    float pad1[16];
    float loss;
    int bad_labels;                    // at ru3d_loss_state_bad_labels_offset(): one read-back path for every loss
    int pad2[2];
};

struct BdWeights {
    float w[RU3D_MAX_CLASSES];      // normalised, slot order
};

extern "C" size_t ru3d_boundary_state_bytes(void) { return sizeof(BdState); }

// not bv_shape_ok alone: nvol volumes of it, every axis within the LDS limit, and the words of all of them an int
static inline bool bd_shape_ok(int nvol, int A, int B, int Z) {
    return nvol > 0 && bv_shape_ok(A, B, Z) && A <= RU3D_BOUNDARY_MAX_AXIS && B <= RU3D_BOUNDARY_MAX_AXIS &&
           Z <= RU3D_BOUNDARY_MAX_AXIS && (int64_t)nvol * A * B * bv_words(Z) < ((int64_t)1 << 31);
}

// the workspace: [flags: nvol unsigned, then the count of bad labels][partials: BD_PART doubles][bits][one int32 plane]
static inline size_t bd_head_bytes(int nvol) { return bv_align(((size_t)nvol + 1) * sizeof(unsigned)); }
static inline size_t bd_part_bytes() { return bv_align((size_t)BD_PART * sizeof(double)); }
static inline size_t bd_bits_bytes(int nvol, int A, int B, int Z) {
    return bv_align((size_t)nvol * A * B * bv_words(Z) * sizeof(bd_u64));
}

extern "C" size_t ru3d_boundary_workspace_bytes(int nvol, int A, int B, int Z) {
    if (!bd_shape_ok(nvol, A, B, Z)) return 0;
    return bd_head_bytes(nvol) + bd_part_bytes() + bd_bits_bytes(nvol, A, B, Z) +
           bv_align((size_t)nvol * A * B * Z * sizeof(int));
}

// columns of z of a tile of an axis of L voxels, as a shift
static inline int bd_tile_shift(int L, int Z) { return bv_tile_shift(L, Z, BD_MAX_COLS, BD_TILE); }

// --------------------------------------------------------------------------- pack
// a wave takes one word a trip; words are numbered (n, a, b, w) with w fastest, so a wave that stays inside one sample
// gathers the flag bits of its words in registers and hands them over once per slot when the sample ends
__global__ __launch_bounds__(256) void bd_pack_kernel(const void* __restrict__ labels, int label_dtype, int64_t rows,
                                                      int64_t rows_per_sample, int Z, int W, int C, ClassList cl,
                                                      bd_u64* __restrict__ bits, unsigned* __restrict__ flags,
                                                      int* __restrict__ bad) {
    const int lane = threadIdx.x & 63;
    const int64_t total = rows * W, step = (int64_t)gridDim.x * 4;
    unsigned seen = 0;                                                      // lane k: the flag bits of slot k
    int64_t seen_n = -1;
    int nbad = 0;
    for (int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < total; i += step) {   // wave-uniform
        const int64_t row = i / W;
        const int w = (int)(i - row * W), z = 64 * w + lane;
        const int64_t n = row / rows_per_sample, r = row - n * rows_per_sample;
        if (n != seen_n) {
            if (lane < cl.K && seen &&
                (__hip_atomic_load(flags + seen_n * cl.K + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & seen) != seen)
                atomicOr(flags + seen_n * cl.K + lane, seen);
            seen = 0;
            seen_n = n;
        }
        const bool in = z < Z;
        const int t = in ? load_label(labels, label_dtype, row * Z + z) : -1;
        const bd_u64 valid = __ballot(in);
        nbad += __popcll(__ballot(in && (t < 0 || t >= C)));
        for (int k = 0; k < cl.K; k++) {
            int c = cl.cls[0];
#pragma unroll
            for (int q = 1; q < RU3D_MAX_CLASSES; q++)
                if (q == k) c = cl.cls[q];
            const bd_u64 word = __ballot(in && t == c);
            if (lane == 0) bits[((n * cl.K + k) * rows_per_sample + r) * W + w] = word;
            if (lane == k) seen |= (word ? 1u : 0u) | ((valid & ~word) ? 2u : 0u);
        }
    }
    // the flag only ever gains bits: a stale read costs one more atomic, never a wrong value
    if (lane < cl.K && seen &&
        (__hip_atomic_load(flags + seen_n * cl.K + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & seen) != seen)
        atomicOr(flags + seen_n * cl.K + lane, seen);
    if (lane == 0 && nbad) atomicAdd(bad, nbad);
}

// --------------------------------------------------------------------------- scans
// distance in voxels from z to the nearest bit of the kind the voxel at z is not, -1 when the row has none: the
// complement is searched for a foreground voxel
__device__ __forceinline__ int bd_nearest(const bd_u64* __restrict__ row, int W, bd_u64 last, int z, bool* fg) {
    const bool me = (row[z >> 6] >> (z & 63)) & 1ull;
    *fg = me;
    return bv_nearest(row, W, last, me ? ~0ull : 0ull, z);
}

// what the candidate `c` costs a voxel whose own value is `me`: nothing when it is of the other kind
__device__ __forceinline__ int bd_cost(int c, int me) { return (c ^ me) < 0 ? 0 : abs(c); }

// min over l' of (l - l')^2 + cost(l') for one output of an [L][T] tile (T = 1 << tshift), with the sign of the voxel
__device__ __forceinline__ int bd_scan(const int* tile, int L, int tshift, int l, int t) {
    const int me = tile[(l << tshift) + t];
    int best = abs(me);
    const int reach = max(l, L - 1 - l);                                    // the hard bound of the scan: reach < L
    for (int d = 1; d <= reach; d++) {
        const int a = d * d;
        if (a >= best) break;                                               // every candidate from here on is >= a
        const int lo = l - d >= 0 ? bd_cost(tile[((l - d) << tshift) + t], me) : BD_BIG;
        const int hi = l + d < L ? bd_cost(tile[((l + d) << tshift) + t], me) : BD_BIG;
        best = min(best, a + min(lo, hi));                                  // a < 2^30 and the cost <= 2^30
    }
    return me < 0 ? -best : best;
}

// does the tile hold anything a background voxel (bit 0) / a foreground voxel (bit 1) could learn from?
__device__ __forceinline__ int bd_tile_info(int info) {
    const int a = __syncthreads_or(info & 1), b = __syncthreads_or(info & 2);
    return (a ? 1 : 0) | (b ? 2 : 0);
}

__global__ __launch_bounds__(BD_THREADS) void bd_zy_kernel(const bd_u64* __restrict__ bits, int nvol, int A, int B, int Z,
                                                           int W, int tshift, int ZT, int* __restrict__ out,
                                                           const unsigned* __restrict__ flags) {
    extern __shared__ int bd_tile[];                                        // [B][T]
    const int T = 1 << tshift, n = B << tshift;
    const bd_u64 last = ~bv_tail(Z);
    const int64_t per_vol = (int64_t)A * ZT, tiles = per_vol * nvol;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t vol = tile / per_vol;
        if (flags[vol] != 3u) continue;                                     // degenerate volume: uniform in the workgroup
        const int64_t r = tile - vol * per_vol;
        const int a = (int)(r / ZT), z0 = (int)(r - (int64_t)a * ZT) << tshift;
        const int64_t plane = vol * A + a;
        int info = 0;
        for (int e = threadIdx.x; e < n; e += BD_THREADS) {
            const int b = e >> tshift, z = z0 + (e & (T - 1));
            int v = BD_BIG;
            if (z < Z) {
                bool fg;
                const int dz = bd_nearest(bits + (plane * B + b) * W, W, last, z, &fg);
                v = dz >= 0 ? dz * dz : BD_BIG;
                if (fg) v = -v;
                info |= (v != BD_BIG ? 1 : 0) | (v != -BD_BIG ? 2 : 0);
            }
            bd_tile[e] = v;
        }
        info = bd_tile_info(info);                                          // uniform from here on; the tile is filled
        for (int e = threadIdx.x; e < n; e += BD_THREADS) {
            const int b = e >> tshift, t = e & (T - 1), z = z0 + t;
            if (z < Z) {
                const int me = bd_tile[e];
                out[(plane * B + b) * Z + z] = (info & (me < 0 ? 2 : 1)) ? bd_scan(bd_tile, B, tshift, b, t) : me;
            }
        }
        __syncthreads();                                                    // the tile is refilled in the next trip
    }
}

__global__ __launch_bounds__(BD_THREADS) void bd_x_kernel(const int* __restrict__ in, int nvol, int A, int B, int Z,
                                                          int tshift, int ZT, int* __restrict__ d2_out,
                                                          float* __restrict__ phi_out,
                                                          const unsigned* __restrict__ flags) {
    extern __shared__ int bd_tile[];                                        // [A][T]
    const int T = 1 << tshift, n = A << tshift;
    const int64_t slab = (int64_t)B * Z, V = slab * A, per_vol = (int64_t)B * ZT, tiles = per_vol * nvol;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t vol = tile / per_vol;
        const int64_t r = tile - vol * per_vol;
        const int b = (int)(r / ZT), z0 = (int)(r - (int64_t)b * ZT) << tshift;
        const int64_t base = vol * V + (int64_t)b * Z;
        const bool live = flags[vol] == 3u;                                 // uniform in the workgroup
        int info = 0;
        if (live) {
            for (int e = threadIdx.x; e < n; e += BD_THREADS) {
                const int a = e >> tshift, z = z0 + (e & (T - 1));
                int v = BD_BIG;
                if (z < Z) {
                    v = in[base + a * slab + z];
                    info |= (v != BD_BIG ? 1 : 0) | (v != -BD_BIG ? 2 : 0);
                }
                bd_tile[e] = v;
            }
            info = bd_tile_info(info);
        }
        for (int e = threadIdx.x; e < n; e += BD_THREADS) {
            const int a = e >> tshift, t = e & (T - 1), z = z0 + t;
            if (z >= Z) continue;
            int s = 0;                                                      // a degenerate volume: no map, no gradient
            if (live) {
                const int me = bd_tile[e];
                s = (info & (me < 0 ? 2 : 1)) ? bd_scan(bd_tile, A, tshift, a, t) : me;
            }
            const int64_t o = base + a * slab + z;
            if (d2_out) d2_out[o] = s;
            if (phi_out) {
                const float root = (float)sqrt((double)abs(s));             // float32(sqrt(d2)), correctly rounded
                phi_out[o] = s < 0 ? -(root - 1.f) : root;
            }
        }
        __syncthreads();
    }
}

// --------------------------------------------------------------------------- the loss
// part[block] = sum over the block's voxels (grid-stride, the grid fixed by the shape) of sum_q w_q P_q phi_q
template <int C>
__global__ __launch_bounds__(256) void bd_loss_kernel(const float* __restrict__ logits, int64_t stride_n,
                                                      int64_t stride_c, int64_t stride_v, int n, int64_t V, ClassList cl,
                                                      BdWeights wt, const float* __restrict__ phi,
                                                      double* __restrict__ part) {
    double acc = 0.0;
    const int64_t total = (int64_t)n * V;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t ni = i / V, vi = i - ni * V;
        float p[C];
        softmax_probs<C>(logits + ni * stride_n + vi * stride_v, stride_c, p);
#pragma unroll
        for (int c = 0; c < C; c++) {
            const int slot = cl.slot[c];
            if (slot >= 0) acc += (double)wt.w[slot] * (double)phi[(ni * cl.K + slot) * V + vi] * (double)p[c];
        }
    }
    __shared__ double sh[4];
    const double r = wave_sum_d(acc);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = r;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// one workgroup: thread t holds partial t (0 beyond `blocks`), ten halving steps in LDS
__global__ __launch_bounds__(BD_PART) void bd_finalize_kernel(const double* __restrict__ part, int blocks, BdWeights wt,
                                                              double inv_count, const int* __restrict__ bad,
                                                              BdState* __restrict__ st, float* __restrict__ loss_out) {
    __shared__ double red[BD_PART];
    red[threadIdx.x] = (int)threadIdx.x < blocks ? part[threadIdx.x] : 0.0;
    __syncthreads();
    for (int h = BD_PART / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    double loss = red[0] * inv_count;
    st->total = red[0];
    for (int k = 0; k < RU3D_MAX_CLASSES; k++) st->w[k] = wt.w[k];
    st->bad_labels = bad[0];
    if (st->bad_labels > 0) loss = nan("");   // F.one_hot would have raised
    st->loss = (float)loss;
    loss_out[0] = (float)loss;
}

// dlogits_j (+)= g / (N V) * P_j * (w_j phi_j [j selected] - sum_q w_q P_q phi_q)
template <int C, bool ACC>
__global__ __launch_bounds__(256) void bd_bwd_kernel(const float* __restrict__ logits, int64_t stride_n, int64_t stride_c,
                                                     int64_t stride_v, int n, int64_t V, ClassList cl,
                                                     const BdState* __restrict__ st, const float* __restrict__ phi,
                                                     const float* __restrict__ grad_out, float scale, float inv_count,
                                                     float* __restrict__ dz) {
    const float go = (grad_out ? grad_out[0] : 1.f) * scale * inv_count;
    float w[C];
#pragma unroll
    for (int c = 0; c < C; c++) {
        w[c] = 0.f;
#pragma unroll
        for (int q = 0; q < RU3D_MAX_CLASSES; q++)
            if (cl.slot[c] == q) w[c] = st->w[q];
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
            const float dp = slot >= 0 ? w[c] * phi[(ni * cl.K + slot) * V + vi] : 0.f;
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

// --------------------------------------------------------------------------- host side
static int bd_check_geom(const char* what, int n, int K, int A, int B, int Z) {
    RU3D_REQUIRE(n > 0 && A > 0 && B > 0 && Z > 0, "%s: empty volume", what);
    RU3D_REQUIRE(A <= RU3D_BOUNDARY_MAX_AXIS && B <= RU3D_BOUNDARY_MAX_AXIS && Z <= RU3D_BOUNDARY_MAX_AXIS,
                 "%s: a %dx%dx%d patch is beyond the limit of %d voxels along an axis (one column of a scanned axis is "
                 "held in LDS and the squares stay exact in float32)", what, A, B, Z, RU3D_BOUNDARY_MAX_AXIS);
    RU3D_REQUIRE((int64_t)n * K < ((int64_t)1 << 31) && bd_shape_ok(n * K, A, B, Z),
                 "%s: a volume of 2^31 voxels or more, or too many volumes", what);
    return 0;
}

static int bd_loss_blocks(int64_t total) {
    int64_t b = (total + BD_PER_BLOCK - 1) / BD_PER_BLOCK;
    if (b > BD_PART) b = BD_PART;
    if (b < 1) b = 1;
    return (int)b;
}

static int bd_flat_blocks(int64_t total) { return flat_bwd_blocks(total, 16384); }

// the whole transform; everything was checked by the caller
static int bd_transform(const void* labels, int label_dtype, int n, int A, int B, int Z, int num_classes,
                        const ClassList& cl, int* d2_out, float* phi_out, void* ws, hipStream_t st) {
    const int nvol = n * cl.K, W = bv_words(Z);
    unsigned* flags = (unsigned*)ws;
    int* bad = (int*)(flags + nvol);
    bd_u64* bits = (bd_u64*)((char*)ws + bd_head_bytes(nvol) + bd_part_bytes());
    int* tmp = (int*)((char*)bits + bd_bits_bytes(nvol, A, B, Z));
    if (hipMemsetAsync(flags, 0, ((size_t)nvol + 1) * sizeof(unsigned), st) != hipSuccess)
        return ru3d_check_launch("signed_distance (memset)");
    const int64_t rows = (int64_t)n * A * B, words = rows * W;
    int64_t pb = (words + 3) / 4;
    if (pb > (int64_t)ru3d_get_cu_budget() * 8) pb = (int64_t)ru3d_get_cu_budget() * 8;
    hipLaunchKernelGGL(bd_pack_kernel, dim3((unsigned)pb), dim3(256), 0, st, labels, label_dtype, rows, (int64_t)A * B, Z,
                       W, num_classes, cl, bits, flags, bad);
    int rc = ru3d_check_launch("signed_distance (pack)");
    if (rc) return rc;
    const int64_t cap = (int64_t)ru3d_get_cu_budget() * 4;                  // four 32 KiB tiles fit a CU's LDS
    {
        const int ts = bd_tile_shift(B, Z), ZT = (Z + (1 << ts) - 1) >> ts;
        const int64_t tiles = (int64_t)nvol * A * ZT;
        hipLaunchKernelGGL(bd_zy_kernel, dim3((unsigned)(tiles < cap ? tiles : cap)), dim3(BD_THREADS),
                           ((size_t)B << ts) * sizeof(int), st, (const bd_u64*)bits, nvol, A, B, Z, W, ts, ZT, tmp,
                           (const unsigned*)flags);
        rc = ru3d_check_launch("signed_distance (zy)");
        if (rc) return rc;
    }
    {
        const int ts = bd_tile_shift(A, Z), ZT = (Z + (1 << ts) - 1) >> ts;
        const int64_t tiles = (int64_t)nvol * B * ZT;
        hipLaunchKernelGGL(bd_x_kernel, dim3((unsigned)(tiles < cap ? tiles : cap)), dim3(BD_THREADS),
                           ((size_t)A << ts) * sizeof(int), st, (const int*)tmp, nvol, A, B, Z, ts, ZT, d2_out, phi_out,
                           (const unsigned*)flags);
    }
    return ru3d_check_launch("signed_distance (x)");
}

extern "C" int ru3d_signed_distance(const void* labels, int label_dtype, int n, int A, int B, int Z, int num_classes,
                                    const int* classes, int num_selected, int32_t* d2_out, float* phi_out, void* ws,
                                    size_t ws_bytes, void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    RU3D_REQUIRE(labels && ws, "signed_distance: null pointer");
    RU3D_REQUIRE(d2_out || phi_out, "signed_distance: null pointer (neither d2_out nor phi_out)");
    RU3D_REQUIRE(label_dtype == RU3D_LABEL_I64 || label_dtype == RU3D_LABEL_U8, "signed_distance: bad label dtype");
    RU3D_REQUIRE(num_classes >= 2 && num_classes <= RU3D_MAX_CLASSES, "signed_distance: %d classes (2 .. %d)", num_classes,
                 RU3D_MAX_CLASSES);
    ClassList cl;
    int rc = class_list_check("signed_distance", num_classes, classes, num_selected, &cl);
    if (rc) return rc;
    rc = bd_check_geom("signed_distance", n, cl.K, A, B, Z);
    if (rc) return rc;
    RU3D_REQUIRE(ws_bytes >= ru3d_boundary_workspace_bytes(n * cl.K, A, B, Z),
                 "signed_distance: workspace of %zu bytes, %zu needed", ws_bytes,
                 ru3d_boundary_workspace_bytes(n * cl.K, A, B, Z));
    return bd_transform(labels, label_dtype, n, A, B, Z, num_classes, cl, (int*)d2_out, phi_out, ws, as_stream(stream));
}

// weight_v restricted to the selected classes over the sum of its absolute values
static BdWeights bd_weights(const float* weight_v, const ClassList& cl) {
    BdWeights wt;
    double wsum = 0.0;
    for (int k = 0; k < cl.K; k++) wsum += fabs(weight_v ? (double)weight_v[cl.cls[k]] : 1.0);
    if (wsum < 1e-12) wsum = 1e-12;
    for (int k = 0; k < RU3D_MAX_CLASSES; k++)
        wt.w[k] = k < cl.K ? (float)((weight_v ? (double)weight_v[cl.cls[k]] : 1.0) / wsum) : 0.f;
    return wt;
}

extern "C" int ru3d_boundary_fwd(const float* logits, int64_t stride_n, int64_t stride_c, int64_t stride_v,
                                 const void* labels, int label_dtype, int n, int A, int B, int Z, int num_classes,
                                 const int* classes, int num_selected, const float* weight_v, float* phi, void* state,
                                 float* loss_out, void* ws, size_t ws_bytes, void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    int rc = loss_view_check("boundary_fwd", logits && labels && phi && state && loss_out && ws,
                             n > 0 && A > 0 && B > 0 && Z > 0, label_dtype, num_classes, 2);
    if (rc) return rc;
    RU3D_REQUIRE(offsetof(BdState, bad_labels) == ru3d_loss_state_bad_labels_offset(),
                 "boundary_fwd: state layouts out of step");
    ClassList cl;
    rc = class_list_check("boundary_fwd", num_classes, classes, num_selected, &cl);
    if (rc) return rc;
    rc = bd_check_geom("boundary_fwd", n, cl.K, A, B, Z);
    if (rc) return rc;
    const int nvol = n * cl.K;
    RU3D_REQUIRE(ws_bytes >= ru3d_boundary_workspace_bytes(nvol, A, B, Z), "boundary_fwd: workspace of %zu bytes, %zu needed",
                 ws_bytes, ru3d_boundary_workspace_bytes(nvol, A, B, Z));
    hipStream_t st = as_stream(stream);
    rc = bd_transform(labels, label_dtype, n, A, B, Z, num_classes, cl, nullptr, phi, ws, st);
    if (rc) return rc;
    const int64_t V = (int64_t)A * B * Z, total = (int64_t)n * V;
    const int blocks = bd_loss_blocks(total);
    double* part = (double*)((char*)ws + bd_head_bytes(nvol));
    const int* bad = (const int*)((const unsigned*)ws + nvol);
    const BdWeights wt = bd_weights(weight_v, cl);
#define CALL(CC)                                                                                                  \
    hipLaunchKernelGGL(bd_loss_kernel<CC>, dim3(blocks), dim3(256), 0, st, logits, stride_n, stride_c, stride_v, n, V, \
                       cl, wt, (const float*)phi, part)
    RU3D_DISPATCH_C(2, num_classes, CALL)
#undef CALL
    rc = ru3d_check_launch("boundary_loss");
    if (rc) return rc;
    hipLaunchKernelGGL(bd_finalize_kernel, dim3(1), dim3(BD_PART), 0, st, (const double*)part, blocks, wt,
                       1.0 / (double)total, bad, (BdState*)state, loss_out);
    return ru3d_check_launch("boundary_finalize");
}

extern "C" int ru3d_boundary_bwd(const float* logits, int64_t stride_n, int64_t stride_c, int64_t stride_v, int n, int A,
                                 int B, int Z, int num_classes, const int* classes, int num_selected, const float* phi,
                                 const void* state, const float* grad_out, float scale, int accumulate, float* dlogits,
                                 void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    // no labels here (the maps of the forward stand for them), so no loss_view_check
    RU3D_REQUIRE(logits && phi && state && dlogits, "boundary_bwd: null pointer");
    RU3D_REQUIRE(num_classes >= 2 && num_classes <= RU3D_MAX_CLASSES, "boundary_bwd: %d classes (2 .. %d)", num_classes,
                 RU3D_MAX_CLASSES);
    ClassList cl;
    int rc = class_list_check("boundary_bwd", num_classes, classes, num_selected, &cl);
    if (rc) return rc;
    rc = bd_check_geom("boundary_bwd", n, cl.K, A, B, Z);
    if (rc) return rc;
    hipStream_t st = as_stream(stream);
    const int64_t V = (int64_t)A * B * Z, total = (int64_t)n * V;
    const float inv_count = (float)(1.0 / (double)total);
#define CALL(CC)                                                                                                       \
    if (accumulate)                                                                                                    \
        hipLaunchKernelGGL((bd_bwd_kernel<CC, true>), dim3(bd_flat_blocks(total)), dim3(256), 0, st, logits, stride_n, \
                           stride_c, stride_v, n, V, cl, (const BdState*)state, phi, grad_out, scale, inv_count,       \
                           dlogits);                                                                                   \
    else                                                                                                               \
        hipLaunchKernelGGL((bd_bwd_kernel<CC, false>), dim3(bd_flat_blocks(total)), dim3(256), 0, st, logits,          \
                           stride_n, stride_c, stride_v, n, V, cl, (const BdState*)state, phi, grad_out, scale,        \
                           inv_count, dlogits)
    RU3D_DISPATCH_C(2, num_classes, CALL)
#undef CALL
    return ru3d_check_launch("boundary_bwd");
}
