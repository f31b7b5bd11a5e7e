// Exact squared Euclidean distance transform of a bit-packed mask, the surface of a packed mask, the gather of a
// float64 volume at the set bits of a packed mask and the reductions the surface-distance metrics need (Hausdorff
// distance, its percentile, average symmetric surface distance, surface Dice).  Packed masks, the nearest-bit walk of
// the Z pass, the tile width and the count / scan / rank pieces of the gather are those of bitvol.h.
//
// The contract of the transform (include/ru3d.h): out[p] = min over the feature voxels f of fl(A + fl(B + C)) with
// A = fl(fl(sx (px - fx))^2), B and C alike for y and z, in float64.  Rounding is monotone, so the separable form
// min_x fl(A + min_y fl(B + min_z C)) has the same bits, and so has any order in which the candidates of one axis are
// visited as long as candidates are compared BY VALUE.  No parabola intersection is computed anywhere; the file is
// compiled with floating-point contraction off, since fl(t * t + c) as one fma is a different number.
//   ed_zy_kernel       Z and Y passes of one x plane and one tile of T columns of z.  The Z pass is read off the packed
//                      words: the nearest set bit below and above z by clz / ctz, walking whole words (at most W of
//                      them), an integer distance per voxel, no byte mask and no float volume in between.  The
//                      [Y][T] tile of C values lives in LDS; every output then scans outward d = 1, 2, ... on both
//                      sides of its y and stops once fl(fl(sy d)^2) alone reaches the best value so far (every later
//                      candidate is at least that).  The scan has a hard bound, d <= max(y, Y - 1 - y) < Y.
//   ed_x_kernel        the same scan along x, in place: a workgroup owns all x of one y and one tile of z columns,
//                      stages them in LDS, synchronises, and writes the results over them.
//                      A tile without a finite value (no feature in it) is written as +inf without a scan, and the X
//                      pass returns at once when the ZY pass met no feature at all (one flag in the workspace).
//   ed_surface_kernel  mask & ~erode(mask) with the 6-neighbour cross and border 0, one word per lane.
//   ed_count / ed_scan / ed_gather   values[r] = sq[p_r] for the set bits p_r of a query mask in element order (x
//                      outermost, z fastest): bitvol.h's compaction over the word popcounts of 256-word chunks, every
//                      lane writes the values of its word at their ranks.
//   ed_reduce_partial / ed_reduce_final   (n, max, #{v <= tau^2}, sum of sqrt(v)) of the first n = min(*count,
//                      capacity) values.  Fixed partition (2048 values per partial whatever the grid) and fixed trees:
//                      the float64 sum has the same bits in every run and under every CU budget.
#include <math.h>
#include "common.h"
#include "bitvol.h"

#pragma clang fp contract(off)

typedef unsigned long long ed_u64;

#define ED_THREADS 512                    // workgroup of the two transform kernels
#define ED_TILE 4096                      // doubles of one LDS tile: 32 KiB, four workgroups a CU
#define ED_MAX_COLS 16                    // columns of z per tile at most: 128-byte segments of the float64 volume
#define ED_GCHUNK 256                     // words of a gather chunk = threads of its workgroup
#define ED_RTHREADS 256
#define ED_RCHUNK 2048                    // values per partial of the reductions

// fl(fl(s d)^2)
__device__ __forceinline__ double ed_sq(double s, int d) {
    const double t = s * (double)d;
    return t * t;
}

// min over l' of fl(fl(fl(s (l - l'))^2) + tile[l'][t]) for one output of an [L][T] tile (T = 1 << tshift)
__device__ __forceinline__ double ed_scan(const double* tile, int L, int tshift, int l, int t, double s) {
    double best = tile[(l << tshift) + t];
    const int reach = max(l, L - 1 - l);                                    // the hard bound of the scan: reach < L
    for (int d = 1; d <= reach; d++) {
        const double a = ed_sq(s, d);
        if (a >= best) break;                                               // every candidate from here on is >= a
        const double lo = l - d >= 0 ? tile[((l - d) << tshift) + t] : INFINITY;
        const double hi = l + d < L ? tile[((l + d) << tshift) + t] : INFINITY;
        best = fmin(best, a + fmin(lo, hi));
    }
    return best;
}

__global__ __launch_bounds__(ED_THREADS) void ed_zy_kernel(const ed_u64* __restrict__ bits, int X, int Y, int Z, int W,
                                                           int tshift, int ZT, double sy, double sz,
                                                           double* __restrict__ out, unsigned* __restrict__ flag) {
    extern __shared__ double ed_tile[];                                     // [Y][T]
    const int T = 1 << tshift, n = Y << tshift;
    const ed_u64 last = ~bv_tail(Z);
    const int64_t tiles = (int64_t)X * ZT;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int x = (int)(tile / ZT), z0 = (int)(tile - (int64_t)x * ZT) << tshift;
        int any = 0;
        for (int e = threadIdx.x; e < n; e += ED_THREADS) {
            const int y = e >> tshift, z = z0 + (e & (T - 1));
            double v = INFINITY;
            if (z < Z) {
                const int dz = bv_nearest(bits + ((int64_t)x * Y + y) * W, W, last, 0ull, z);
                if (dz >= 0) {
                    v = ed_sq(sz, dz);
                    any = 1;
                }
            }
            ed_tile[e] = v;
        }
        any = __syncthreads_or(any);                                        // uniform from here on
        for (int e = threadIdx.x; e < n; e += ED_THREADS) {
            const int y = e >> tshift, t = e & (T - 1), z = z0 + t;
            if (z < Z) out[((int64_t)x * Y + y) * Z + z] = any ? ed_scan(ed_tile, Y, tshift, y, t, sy) : INFINITY;
        }
        if (any && threadIdx.x == 0) atomicOr(flag, 1u);
        __syncthreads();                                                    // the tile is refilled in the next trip
    }
}

__global__ __launch_bounds__(ED_THREADS) void ed_x_kernel(double* __restrict__ out, int X, int Y, int Z, int tshift, int ZT,
                                                          double sx, const unsigned* __restrict__ flag) {
    extern __shared__ double ed_tile[];                                     // [X][T]
    if (*flag == 0) return;                                                 // no feature anywhere: out is +inf already
    const int T = 1 << tshift, n = X << tshift;
    const int64_t plane = (int64_t)Y * Z, tiles = (int64_t)Y * ZT;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int y = (int)(tile / ZT), z0 = (int)(tile - (int64_t)y * ZT) << tshift;
        int any = 0;
        for (int e = threadIdx.x; e < n; e += ED_THREADS) {
            const int x = e >> tshift, z = z0 + (e & (T - 1));
            const double v = z < Z ? out[x * plane + (int64_t)y * Z + z] : INFINITY;
            any |= v < INFINITY;
            ed_tile[e] = v;
        }
        any = __syncthreads_or(any);                                        // and every read of the column is done
        if (any) {
            for (int e = threadIdx.x; e < n; e += ED_THREADS) {
                const int x = e >> tshift, t = e & (T - 1), z = z0 + t;
                if (z < Z) out[x * plane + (int64_t)y * Z + z] = ed_scan(ed_tile, X, tshift, x, t, sx);
            }
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------ surface
__global__ __launch_bounds__(256) void ed_surface_kernel(const ed_u64* __restrict__ src, ed_u64* __restrict__ dst, int X,
                                                         int Y, int Z, int W, int64_t words) {
    const ed_u64 tail = bv_tail(Z);
    const int64_t xstep = (int64_t)Y * W;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < words; i += (int64_t)gridDim.x * 256) {
        const int64_t row = i / W;
        const int w = (int)(i - row * W), y = (int)(row % Y), x = (int)(row / Y);
        const ed_u64 m = w == W - 1 ? src[i] & ~tail : src[i];
        ed_u64 e = 0;
        if (m && x > 0 && x < X - 1 && y > 0 && y < Y - 1) {                // a face voxel has a neighbour outside: 0
            const ed_u64 below = w > 0 ? src[i - 1] : 0ull;
            const ed_u64 above = w < W - 1 ? (w + 1 == W - 1 ? src[i + 1] & ~tail : src[i + 1]) : 0ull;
            e = m & bv_zdown(below, m) & bv_zup(m, above);                  // z - 1 and z + 1
            e &= src[i - xstep] & src[i + xstep] & src[i - W] & src[i + W];
        }
        dst[i] = m & ~e;
    }
}

// ------------------------------------------------------------------------------------------------ gather
__device__ __forceinline__ ed_u64 ed_query_word(const ed_u64* __restrict__ q, int64_t i, int64_t words, int W, ed_u64 tail) {
    if (i >= words) return 0ull;
    return (i % W) == W - 1 ? q[i] & ~tail : q[i];
}

__global__ __launch_bounds__(ED_GCHUNK) void ed_count_kernel(const ed_u64* __restrict__ q, int64_t words, int W, ed_u64 tail,
                                                             int* __restrict__ counts) {
    bv_chunk_sum(__popcll(ed_query_word(q, (int64_t)blockIdx.x * ED_GCHUNK + threadIdx.x, words, W, tail)), counts);
}

// bv_scan_chunks over the chunk counts, the total -> *total
__global__ __launch_bounds__(BV_SCAN_THREADS) void ed_scan_kernel(int* __restrict__ counts, int chunks,
                                                                  long long* __restrict__ total) {
    __shared__ int s_sum[BV_SCAN_THREADS];
    const int sum = bv_scan_chunks(counts, chunks, s_sum);
    if (threadIdx.x == BV_SCAN_THREADS - 1) *total = (long long)sum;
}

__global__ __launch_bounds__(ED_GCHUNK) void ed_gather_kernel(const double* __restrict__ sq, const ed_u64* __restrict__ q,
                                                              int64_t words, int W, int Z, ed_u64 tail,
                                                              const int* __restrict__ offsets, double* __restrict__ values,
                                                              long long capacity) {
    const int64_t i = (int64_t)blockIdx.x * ED_GCHUNK + threadIdx.x;
    ed_u64 m = ed_query_word(q, i, words, W, tail);
    long long rank = (long long)offsets[blockIdx.x] + bv_chunk_rank(__popcll(m));
    if (!m) return;
    const int64_t row = i / W;
    const double* base = sq + row * Z + 64 * (int)(i - row * W);
    while (m) {                                                             // at most 64 trips: one per set bit
        const int b = __ffsll(m) - 1;
        m &= m - 1;
        if (rank < capacity) values[rank] = base[b];
        rank++;
    }
}

// ------------------------------------------------------------------------------------------------ reductions
struct ed_stats {
    double mx, cnt, sum;
};
__device__ __forceinline__ ed_stats ed_join(const ed_stats& a, const ed_stats& b) {
    ed_stats r = {fmax(a.mx, b.mx), a.cnt + b.cnt, a.sum + b.sum};
    return r;
}
// the workgroup's total in thread 0, in bv_block_join's fixed order
__device__ __forceinline__ ed_stats ed_block_join(ed_stats v, ed_stats* s_part) {
    return bv_block_join(v, s_part, [](const ed_stats& a, const ed_stats& b) { return ed_join(a, b); });
}
__device__ __forceinline__ long long ed_used(const long long* count, long long capacity) {
    const long long c = *count;
    return c < 0 ? 0 : (c < capacity ? c : capacity);
}

__global__ __launch_bounds__(ED_RTHREADS) void ed_reduce_partial_kernel(const double* __restrict__ values,
                                                                        const long long* __restrict__ count,
                                                                        long long capacity, double tau_sq,
                                                                        double* __restrict__ partial) {
    __shared__ ed_stats s_part[ED_RTHREADS / 64];
    const long long n = ed_used(count, capacity), chunks = (n + ED_RCHUNK - 1) / ED_RCHUNK;
    for (long long chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
        ed_stats v = {0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < ED_RCHUNK / ED_RTHREADS; k++) {
            const long long i = chunk * ED_RCHUNK + k * ED_RTHREADS + threadIdx.x;
            if (i < n) {
                const double x = values[i];
                v.mx = fmax(v.mx, x);
                v.cnt += x <= tau_sq ? 1.0 : 0.0;
                v.sum += sqrt(x);
            }
        }
        v = ed_block_join(v, s_part);
        if (threadIdx.x == 0) {
            partial[3 * chunk] = v.mx;
            partial[3 * chunk + 1] = v.cnt;
            partial[3 * chunk + 2] = v.sum;
        }
    }
}

__global__ __launch_bounds__(ED_RTHREADS) void ed_reduce_final_kernel(const double* __restrict__ partial,
                                                                      const long long* __restrict__ count,
                                                                      long long capacity, double* __restrict__ out) {
    __shared__ ed_stats s_part[ED_RTHREADS / 64];
    const long long n = ed_used(count, capacity), chunks = (n + ED_RCHUNK - 1) / ED_RCHUNK;
    ed_stats v = {0.0, 0.0, 0.0};
    for (long long chunk = threadIdx.x; chunk < chunks; chunk += ED_RTHREADS) {
        ed_stats w = {partial[3 * chunk], partial[3 * chunk + 1], partial[3 * chunk + 2]};
        v = ed_join(v, w);
    }
    v = ed_block_join(v, s_part);
    if (threadIdx.x == 0) {
        out[0] = (double)n;
        out[1] = v.mx;
        out[2] = v.cnt;
        out[3] = v.sum;
    }
}

// ------------------------------------------------------------------------------------------------ host side
// columns of z of a tile of an axis of L voxels, as a shift
static inline int ed_tile_shift(int L, int Z) { return bv_tile_shift(L, Z, ED_MAX_COLS, ED_TILE); }

extern "C" size_t ru3d_edt_workspace_bytes(int X, int Y, int Z) {
    if (!bv_shape_ok(X, Y, Z) || X > RU3D_EDT_MAX_AXIS || Y > RU3D_EDT_MAX_AXIS) return 0;
    return bv_align(sizeof(unsigned));
}

extern "C" int ru3d_edt_squared(const uint64_t* bits, int X, int Y, int Z, const double* spacing, double* out, void* ws,
                                size_t ws_bytes, void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    BV_REQUIRE_SHAPE("edt_squared");
    RU3D_REQUIRE(X <= RU3D_EDT_MAX_AXIS && Y <= RU3D_EDT_MAX_AXIS,
                 "edt_squared: a %dx%dx%d volume is beyond the limit of %d voxels along x and y (one column of the axis "
                 "is held in LDS)", X, Y, Z, RU3D_EDT_MAX_AXIS);
    RU3D_REQUIRE(bits && spacing && out && ws, "edt_squared: bad argument (null pointer)");
    for (int a = 0; a < 3; a++)
        RU3D_REQUIRE(isfinite(spacing[a]) && spacing[a] > 0.0, "edt_squared: spacing[%d] = %g (finite and > 0)", a,
                     spacing[a]);
    RU3D_REQUIRE(ws_bytes >= ru3d_edt_workspace_bytes(X, Y, Z), "edt_squared: workspace of %zu bytes, %zu needed", ws_bytes,
                 ru3d_edt_workspace_bytes(X, Y, Z));
    hipStream_t st = as_stream(stream);
    unsigned* flag = (unsigned*)ws;
    if (hipMemsetAsync(flag, 0, sizeof(unsigned), st) != hipSuccess) return ru3d_check_launch("edt_squared (memset)");
    const int64_t cap = (int64_t)ru3d_get_cu_budget() * 4;                  // four 32 KiB tiles fit a CU's LDS
    {
        const int ts = ed_tile_shift(Y, Z), ZT = (Z + (1 << ts) - 1) >> ts;
        const int64_t tiles = (int64_t)X * ZT;
        hipLaunchKernelGGL(ed_zy_kernel, dim3((unsigned)(tiles < cap ? tiles : cap)), dim3(ED_THREADS),
                           ((size_t)Y << ts) * sizeof(double), st, (const ed_u64*)bits, X, Y, Z, bv_words(Z), ts, ZT,
                           spacing[1], spacing[2], out, flag);
    }
    if (X > 1) {
        const int ts = ed_tile_shift(X, Z), ZT = (Z + (1 << ts) - 1) >> ts;
        const int64_t tiles = (int64_t)Y * ZT;
        hipLaunchKernelGGL(ed_x_kernel, dim3((unsigned)(tiles < cap ? tiles : cap)), dim3(ED_THREADS),
                           ((size_t)X << ts) * sizeof(double), st, out, X, Y, Z, ts, ZT, spacing[0],
                           (const unsigned*)flag);
    }
    return ru3d_check_launch("edt_squared");
}

extern "C" int ru3d_mask_surface(const uint64_t* src, uint64_t* dst, int X, int Y, int Z, void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    BV_REQUIRE_SHAPE("mask_surface");
    RU3D_REQUIRE(src && dst, "mask_surface: bad argument (null pointer)");
    RU3D_REQUIRE(src != dst, "mask_surface: not an in-place operation (src == dst)");
    const int W = bv_words(Z);
    const int64_t words = (int64_t)X * Y * W, cap = (int64_t)ru3d_get_cu_budget() * 8;
    int64_t blocks = (words + 255) / 256;
    blocks = blocks > cap ? cap : blocks;
    hipLaunchKernelGGL(ed_surface_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), (const ed_u64*)src,
                       (ed_u64*)dst, X, Y, Z, W, words);
    return ru3d_check_launch("mask_surface");
}

extern "C" size_t ru3d_edt_gather_workspace_bytes(int X, int Y, int Z) {
    if (!bv_shape_ok(X, Y, Z)) return 0;
    const int64_t words = (int64_t)X * Y * bv_words(Z);
    return bv_align((size_t)((words + ED_GCHUNK - 1) / ED_GCHUNK) * sizeof(int));
}

extern "C" int ru3d_edt_gather(const double* sq, const uint64_t* query, int X, int Y, int Z, double* values,
                               int64_t capacity, int64_t* count, void* ws, size_t ws_bytes, void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    BV_REQUIRE_SHAPE("edt_gather");
    RU3D_REQUIRE(query && count && ws && (sq || !values), "edt_gather: bad argument (null pointer)");
    RU3D_REQUIRE(!values || capacity >= 1, "edt_gather: capacity %lld of the output buffer (>= 1)", (long long)capacity);
    RU3D_REQUIRE(ws_bytes >= ru3d_edt_gather_workspace_bytes(X, Y, Z), "edt_gather: workspace of %zu bytes, %zu needed",
                 ws_bytes, ru3d_edt_gather_workspace_bytes(X, Y, Z));
    hipStream_t st = as_stream(stream);
    const int W = bv_words(Z);
    const int64_t words = (int64_t)X * Y * W;
    const int chunks = (int)((words + ED_GCHUNK - 1) / ED_GCHUNK);
    int* counts = (int*)ws;
    hipLaunchKernelGGL(ed_count_kernel, dim3(chunks), dim3(ED_GCHUNK), 0, st, (const ed_u64*)query, words, W, bv_tail(Z),
                       counts);
    hipLaunchKernelGGL(ed_scan_kernel, dim3(1), dim3(BV_SCAN_THREADS), 0, st, counts, chunks, (long long*)count);
    if (values)
        hipLaunchKernelGGL(ed_gather_kernel, dim3(chunks), dim3(ED_GCHUNK), 0, st, sq, (const ed_u64*)query, words, W, Z,
                           bv_tail(Z), (const int*)counts, values, (long long)capacity);
    return ru3d_check_launch("edt_gather");
}

extern "C" size_t ru3d_edt_reduce_workspace_bytes(int64_t capacity) {
    if (capacity < 1 || capacity >= ((int64_t)1 << 40)) return 0;
    return bv_align((size_t)((capacity + ED_RCHUNK - 1) / ED_RCHUNK) * 3 * sizeof(double));
}

extern "C" int ru3d_edt_reduce(const double* values, const int64_t* count, int64_t capacity, double tau_sq, double* out,
                               void* ws, size_t ws_bytes, void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    RU3D_REQUIRE(capacity >= 1 && capacity < ((int64_t)1 << 40), "edt_reduce: capacity %lld (1 .. 2^40 - 1)",
                 (long long)capacity);
    RU3D_REQUIRE(values && count && out && ws, "edt_reduce: bad argument (null pointer)");
    RU3D_REQUIRE(!isnan(tau_sq) && tau_sq >= 0.0, "edt_reduce: squared tolerance %g (>= 0)", tau_sq);
    RU3D_REQUIRE(ws_bytes >= ru3d_edt_reduce_workspace_bytes(capacity), "edt_reduce: workspace of %zu bytes, %zu needed",
                 ws_bytes, ru3d_edt_reduce_workspace_bytes(capacity));
    hipStream_t st = as_stream(stream);
    const int64_t chunks = (capacity + ED_RCHUNK - 1) / ED_RCHUNK, cap = (int64_t)ru3d_get_cu_budget() * 8;
    hipLaunchKernelGGL(ed_reduce_partial_kernel, dim3((unsigned)(chunks < cap ? chunks : cap)), dim3(ED_RTHREADS), 0, st,
                       values, (const long long*)count, (long long)capacity, tau_sq, (double*)ws);
    hipLaunchKernelGGL(ed_reduce_final_kernel, dim3(1), dim3(ED_RTHREADS), 0, st, (const double*)ws,
                       (const long long*)count, (long long)capacity, out);
    return ru3d_check_launch("edt_reduce");
}
