// Nearest site and territories: the exact Euclidean feature transform of a bit-packed mask (which set voxel is nearest,
// and how far), the labels of a region by nearest site, and the integer tally of those labels against a second label
// volume.  Packed masks, the tile width and the count / scan / rank pieces are those of bitvol.h; the launch shape
// (persistent tile loops under the CU budget) and the arithmetic are those of distance.hip.
//
// The contract (include/ru3d.h, "nearest site / territories"): the squared distance has the bits of ru3d_edt_squared,
// min over the sites f of fl(A + fl(B + C)); the site is chosen separably, by value, with the smaller coordinate
// winning a tie on every axis.  The file is compiled with floating-point contraction off, as distance.hip is.
//   tr_zy_kernel       Z and Y passes of one x plane and one tile of T columns of z.  The Z pass reads the nearest set bit
//                      at or below and at or above z off the packed words and takes the lower one when both are equally
//                      far.  Two LDS tiles, [Y][T] float64 values and [Y][T] int32 sites (the z of the chosen bit); every
//                      output scans outward d = 1, 2, ... and stops once fl(fl(sy d)^2) alone EXCEEDS the best value - a
//                      candidate on the low side that only ties the best still has to win, so the scan runs on while
//                      a == best.  Per d the low side is compared first with <=, the high side with <: every candidate
//                      met earlier has a larger coordinate than the low one and a smaller one than the high one.
//   tr_x_kernel        the same scan along x, in place on both volumes: a workgroup owns all x of one y and one tile of z
//                      columns, stages values and sites (y' Z + z') in LDS, synchronises, and writes the results over them.
//                      A tile without a finite value is left as the ZY pass wrote it (+inf, -1); the X pass returns at
//                      once when the ZY pass met no site at all (one flag in the workspace).
//   tr_count / tr_scan / tr_prefix   per word of the site mask, the number of set bits in front of it in element order.
//   tr_assign_kernel   labels[p] = site_ids[rank(index[p])] on the region.
//   tr_tally_kernel    table[label][min(other, num_other)] += 1 on the region: 32-bit counters in LDS per workgroup when
//                      the table fits TR_LDS_CELLS, flushed with 64-bit atomics; 64-bit atomics to the table otherwise.
// What only the device can see (a count of sites that is not n, an index that is no site, a label outside 0 .. K) sets a
// bit of an error word in the workspace; the entry point reads the word back once, after its launches, and returns -2.
#include <math.h>
#include "common.h"
#include "bitvol.h"

#pragma clang fp contract(off)

typedef unsigned long long tr_u64;

#define TR_THREADS 512                    // workgroup of the two transform kernels
#define TR_TILE 4096                      // elements of one LDS tile: 32 KiB of values + 16 KiB of sites
#define TR_MAX_COLS 16                    // columns of z per tile at most
#define TR_TILES_PER_CU 3                 // 48 KiB a workgroup in 160 KiB of LDS
#define TR_CHUNK BV_CHUNK_THREADS         // words of a rank chunk = threads of its workgroup
#define TR_LDS_CELLS 8192                 // 32-bit counters of a workgroup's tally table: 32 KiB
#define TR_ERR_COUNT 1u                   // the site mask does not have n set bits
#define TR_ERR_INDEX 2u                   // an index that is not a set bit of the site mask
#define TR_ERR_LABEL 4u                   // a label outside 0 .. K

// fl(fl(s d)^2)
__device__ __forceinline__ double tr_sq(double s, int d) {
    const double t = s * (double)d;
    return t * t;
}

// z of the nearest set bit of a packed row, the lower one of two that are equally far; -1 when there is none.
// last: the bits at z < Z of the row's last word (~bv_tail)
__device__ __forceinline__ int tr_nearest_z(const tr_u64* __restrict__ row, int W, tr_u64 last, int z) {
    const int w = z >> 6, b = z & 63;
    const tr_u64 cur = row[w] & (w == W - 1 ? last : ~0ull);
    int lo = -1, hi = -1;
    tr_u64 m = cur & (~0ull >> (63 - b));                                   // the bits at or below z
    if (m) {
        lo = 64 * w + 63 - __clzll(m);
    } else {
        for (int k = w - 1; k >= 0; k--) {
            const tr_u64 v = row[k];
            if (v) {
                lo = 64 * k + 63 - __clzll(v);
                break;
            }
        }
    }
    m = cur & (~0ull << b);                                                 // the bits at or above z
    if (m) {
        hi = 64 * w + __ffsll(m) - 1;
    } else {
        for (int k = w + 1; k < W; k++) {
            const tr_u64 v = row[k] & (k == W - 1 ? last : ~0ull);
            if (v) {
                hi = 64 * k + __ffsll(v) - 1;
                break;
            }
        }
    }
    if (lo < 0) return hi;
    if (hi < 0) return lo;
    return z - lo <= hi - z ? lo : hi;
}

// min over l' of fl(fl(fl(s (l - l'))^2) + val[l'][t]) for one output of an [L][T] tile (T = 1 << tshift), and in *at
// the smallest l' that attains it
__device__ __forceinline__ double tr_scan(const double* val, int L, int tshift, int l, int t, double s, int* at) {
    double best = val[(l << tshift) + t];
    int arg = l;
    const int reach = max(l, L - 1 - l);                                    // the hard bound of the scan: reach < L
    for (int d = 1; d <= reach; d++) {
        const double a = tr_sq(s, d);
        if (a > best) break;                                                // every candidate from here on is > best
        if (l - d >= 0) {
            const double v = a + val[((l - d) << tshift) + t];
            if (v <= best) {                                                // a smaller coordinate than any met so far
                best = v;
                arg = l - d;
            }
        }
        if (l + d < L) {
            const double v = a + val[((l + d) << tshift) + t];
            if (v < best) {
                best = v;
                arg = l + d;
            }
        }
    }
    *at = arg;
    return best;
}

__global__ __launch_bounds__(TR_THREADS) void tr_zy_kernel(const tr_u64* __restrict__ bits, int X, int Y, int Z, int W,
                                                           int tshift, int ZT, double sy, double sz,
                                                           double* __restrict__ out, int* __restrict__ index,
                                                           unsigned* __restrict__ flag) {
    extern __shared__ double tr_tile[];                                     // [Y][T] values, then [Y][T] sites
    const int T = 1 << tshift, n = Y << tshift;
    int* tr_site = (int*)(tr_tile + n);
    const tr_u64 last = ~bv_tail(Z);
    const int64_t tiles = (int64_t)X * ZT;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int x = (int)(tile / ZT), z0 = (int)(tile - (int64_t)x * ZT) << tshift;
        int any = 0;
        for (int e = threadIdx.x; e < n; e += TR_THREADS) {
            const int y = e >> tshift, z = z0 + (e & (T - 1));
            double v = INFINITY;
            int site = -1;
            if (z < Z) {
                site = tr_nearest_z(bits + ((int64_t)x * Y + y) * W, W, last, z);
                if (site >= 0) {
                    v = tr_sq(sz, site > z ? site - z : z - site);
                    any = 1;
                }
            }
            tr_tile[e] = v;
            tr_site[e] = site;
        }
        any = __syncthreads_or(any);                                        // uniform from here on
        for (int e = threadIdx.x; e < n; e += TR_THREADS) {
            const int y = e >> tshift, t = e & (T - 1), z = z0 + t;
            if (z >= Z) continue;
            double v = INFINITY;
            int site = -1;
            if (any) {
                int at;
                v = tr_scan(tr_tile, Y, tshift, y, t, sy, &at);
                if (v < INFINITY) site = at * Z + tr_site[(at << tshift) + t];
            }
            const int64_t p = ((int64_t)x * Y + y) * Z + z;
            out[p] = v;
            index[p] = site;
        }
        if (any && threadIdx.x == 0) atomicOr(flag, 1u);
        __syncthreads();                                                    // the tiles are refilled in the next trip
    }
}

__global__ __launch_bounds__(TR_THREADS) void tr_x_kernel(double* __restrict__ out, int* __restrict__ index, int X, int Y,
                                                          int Z, int tshift, int ZT, double sx,
                                                          const unsigned* __restrict__ flag) {
    extern __shared__ double tr_tile[];                                     // [X][T] values, then [X][T] sites
    if (*flag == 0) return;                                                 // no site anywhere: +inf and -1 already
    const int T = 1 << tshift, n = X << tshift;
    int* tr_site = (int*)(tr_tile + n);
    const int64_t plane = (int64_t)Y * Z, tiles = (int64_t)Y * ZT;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int y = (int)(tile / ZT), z0 = (int)(tile - (int64_t)y * ZT) << tshift;
        int any = 0;
        for (int e = threadIdx.x; e < n; e += TR_THREADS) {
            const int x = e >> tshift, z = z0 + (e & (T - 1));
            double v = INFINITY;
            int site = -1;
            if (z < Z) {
                const int64_t p = x * plane + (int64_t)y * Z + z;
                v = out[p];
                site = index[p];
            }
            any |= v < INFINITY;
            tr_tile[e] = v;
            tr_site[e] = site;
        }
        any = __syncthreads_or(any);                                        // and every read of the column is done
        if (any) {
            for (int e = threadIdx.x; e < n; e += TR_THREADS) {
                const int x = e >> tshift, t = e & (T - 1), z = z0 + t;
                if (z >= Z) continue;
                int at;
                const double v = tr_scan(tr_tile, X, tshift, x, t, sx, &at);
                const int64_t p = x * plane + (int64_t)y * Z + z;
                out[p] = v;
                index[p] = v < INFINITY ? (int)(at * plane) + tr_site[(at << tshift) + t] : -1;
            }
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------ ranks of the sites
__device__ __forceinline__ tr_u64 tr_site_word(const tr_u64* __restrict__ q, int64_t i, int64_t words, int W, tr_u64 tail) {
    if (i >= words) return 0ull;
    return (i % W) == W - 1 ? q[i] & ~tail : q[i];
}

__global__ __launch_bounds__(TR_CHUNK) void tr_count_kernel(const tr_u64* __restrict__ q, int64_t words, int W, tr_u64 tail,
                                                            int* __restrict__ counts) {
    bv_chunk_sum(__popcll(tr_site_word(q, (int64_t)blockIdx.x * TR_CHUNK + threadIdx.x, words, W, tail)), counts);
}

// bv_scan_chunks over the chunk counts; a total that is not n sets TR_ERR_COUNT
__global__ __launch_bounds__(BV_SCAN_THREADS) void tr_scan_kernel(int* __restrict__ counts, int chunks, long long n,
                                                                  unsigned* __restrict__ err) {
    __shared__ long long s_sum[BV_SCAN_THREADS];
    const long long sum = bv_scan_chunks(counts, chunks, s_sum);
    if (threadIdx.x == 0 && sum != n) atomicOr(err, TR_ERR_COUNT);
}

// prefix[i] = the set bits of the words in front of word i
__global__ __launch_bounds__(TR_CHUNK) void tr_prefix_kernel(const tr_u64* __restrict__ q, int64_t words, int W, tr_u64 tail,
                                                             const int* __restrict__ offsets, int* __restrict__ prefix) {
    const int64_t i = (int64_t)blockIdx.x * TR_CHUNK + threadIdx.x;
    const int rank = offsets[blockIdx.x] + bv_chunk_rank(__popcll(tr_site_word(q, i, words, W, tail)));
    if (i < words) prefix[i] = rank;
}

__device__ __forceinline__ bool tr_in_region(const tr_u64* __restrict__ region, int W, unsigned row, unsigned z) {
    return !region || ((region[(int64_t)row * W + (z >> 6)] >> (z & 63)) & 1ull);
}

__global__ __launch_bounds__(256) void tr_assign_kernel(const tr_u64* __restrict__ sites, const tr_u64* __restrict__ region,
                                                        const int* __restrict__ index, const int* __restrict__ site_ids,
                                                        long long n, int Z, int W, int64_t voxels,
                                                        const int* __restrict__ prefix, int* __restrict__ labels,
                                                        unsigned* __restrict__ err) {
    const bool counted = !(*(volatile unsigned*)err & TR_ERR_COUNT);         // set by tr_scan_kernel, a launch earlier
    unsigned bad = 0;
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < voxels; p += (int64_t)gridDim.x * 256) {
        const unsigned row = (unsigned)p / (unsigned)Z, z = (unsigned)p - row * (unsigned)Z;
        int label = 0;
        if (counted && tr_in_region(region, W, row, z)) {
            const int f = index[p];
            if (f >= voxels) {
                bad = TR_ERR_INDEX;
            } else if (f >= 0) {
                const unsigned frow = (unsigned)f / (unsigned)Z, fz = (unsigned)f - frow * (unsigned)Z;
                const int64_t word = (int64_t)frow * W + (fz >> 6);
                const tr_u64 m = sites[word];                               // fz < Z: never a tail bit
                const long long rank = (long long)prefix[word] + __popcll(m & ((1ull << (fz & 63)) - 1ull));
                if (((m >> (fz & 63)) & 1ull) && rank < n) label = site_ids[rank];
                else bad = TR_ERR_INDEX;
            }
        }
        labels[p] = label;
    }
    if (bad) atomicOr(err, bad);
}

// ------------------------------------------------------------------------------------------------ tally
template <bool LDS>
__global__ __launch_bounds__(256) void tr_tally_kernel(const int* __restrict__ labels, int K, const uint8_t* __restrict__ other,
                                                       int num_other, const tr_u64* __restrict__ region, int Z, int W,
                                                       int64_t voxels, unsigned long long* __restrict__ table,
                                                       unsigned* __restrict__ err) {
    __shared__ unsigned s_table[LDS ? TR_LDS_CELLS : 1];
    const int cols = num_other + 1, cells = LDS ? (K + 1) * cols : 0;       // LDS: cells <= TR_LDS_CELLS
    if (LDS) {
        for (int c = threadIdx.x; c < cells; c += 256) s_table[c] = 0u;
        __syncthreads();
    }
    unsigned bad = 0;
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < voxels; p += (int64_t)gridDim.x * 256) {
        const unsigned row = (unsigned)p / (unsigned)Z, z = (unsigned)p - row * (unsigned)Z;
        if (!tr_in_region(region, W, row, z)) continue;
        const int l = labels[p];
        if (l < 0 || l > K) {
            bad = TR_ERR_LABEL;
            continue;
        }
        const int o = other ? min((int)other[p], num_other) : 0;
        if (LDS) atomicAdd(&s_table[l * cols + o], 1u);                      // fewer than 2^31 voxels in all: no overflow
        else atomicAdd(&table[(int64_t)l * cols + o], 1ull);
    }
    if (LDS) {
        __syncthreads();
        for (int c = threadIdx.x; c < cells; c += 256) {
            const unsigned v = s_table[c];
            if (v) atomicAdd(&table[c], (unsigned long long)v);
        }
    }
    if (bad) atomicOr(err, bad);
}

// ------------------------------------------------------------------------------------------------ host side
static inline int tr_tile_shift(int L, int Z) { return bv_tile_shift(L, Z, TR_MAX_COLS, TR_TILE); }

// the error word of an entry point, read back after its launches: 0, or a negative status with the message set
static int tr_read_errors(const char* what, unsigned* err, hipStream_t st) {
    unsigned bits = 0;
    if (hipMemcpyAsync(&bits, err, sizeof(bits), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) {
        ru3d_check_launch(what);
        return ru3d_fail(-1, "%s: reading the error word back failed", what);
    }
    if (bits & TR_ERR_COUNT) return ru3d_fail(-2, "%s: n is not the number of set bits of the site mask", what);
    if (bits & TR_ERR_INDEX) return ru3d_fail(-2, "%s: an index that is not a set voxel of the site mask", what);
    if (bits & TR_ERR_LABEL) return ru3d_fail(-2, "%s: a label outside 0 .. K", what);
    return 0;
}

// the flag of ru3d_edt_squared, and the float64 volume when the caller wants none back
static size_t tr_nearest_workspace_bytes(int X, int Y, int Z, bool with_sq) {
    return ru3d_edt_workspace_bytes(X, Y, Z) + (with_sq ? 0 : (size_t)X * Y * Z * sizeof(double));
}

extern "C" int ru3d_nearest_site(const uint64_t* bits, int X, int Y, int Z, const double* spacing, int32_t* index, double* sq,
                                 void* ws, size_t ws_bytes, void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    BV_REQUIRE_SHAPE("nearest_site");
    RU3D_REQUIRE(X <= RU3D_EDT_MAX_AXIS && Y <= RU3D_EDT_MAX_AXIS,
                 "nearest_site: a %dx%dx%d volume is beyond the limit of %d voxels along x and y (one column of the axis "
                 "is held in LDS)", X, Y, Z, RU3D_EDT_MAX_AXIS);
    RU3D_REQUIRE(bits && spacing && index && ws, "nearest_site: bad argument (null pointer)");
    for (int a = 0; a < 3; a++)
        RU3D_REQUIRE(isfinite(spacing[a]) && spacing[a] > 0.0, "nearest_site: spacing[%d] = %g (finite and > 0)", a,
                     spacing[a]);
    const size_t need = tr_nearest_workspace_bytes(X, Y, Z, sq != NULL);
    RU3D_REQUIRE(ws_bytes >= need, "nearest_site: workspace of %zu bytes, %zu needed", ws_bytes, need);
    hipStream_t st = as_stream(stream);
    unsigned* flag = (unsigned*)ws;
    double* out = sq ? sq : (double*)((char*)ws + ru3d_edt_workspace_bytes(X, Y, Z));
    if (hipMemsetAsync(flag, 0, sizeof(unsigned), st) != hipSuccess) return ru3d_check_launch("nearest_site (memset)");
    const int64_t cap = (int64_t)ru3d_get_cu_budget() * TR_TILES_PER_CU;
    {
        const int ts = tr_tile_shift(Y, Z), ZT = (Z + (1 << ts) - 1) >> ts;
        const int64_t tiles = (int64_t)X * ZT;
        hipLaunchKernelGGL(tr_zy_kernel, dim3((unsigned)(tiles < cap ? tiles : cap)), dim3(TR_THREADS),
                           ((size_t)Y << ts) * (sizeof(double) + sizeof(int)), st, (const tr_u64*)bits, X, Y, Z, bv_words(Z),
                           ts, ZT, spacing[1], spacing[2], out, (int*)index, flag);
    }
    if (X > 1) {
        const int ts = tr_tile_shift(X, Z), ZT = (Z + (1 << ts) - 1) >> ts;
        const int64_t tiles = (int64_t)Y * ZT;
        hipLaunchKernelGGL(tr_x_kernel, dim3((unsigned)(tiles < cap ? tiles : cap)), dim3(TR_THREADS),
                           ((size_t)X << ts) * (sizeof(double) + sizeof(int)), st, out, (int*)index, X, Y, Z, ts, ZT,
                           spacing[0], (const unsigned*)flag);
    }
    return ru3d_check_launch("nearest_site");
}

// the error word, a count per chunk and a prefix per word: less than the two planes of packed words the caller brings
static size_t tr_assign_carved_bytes(int X, int Y, int Z) {
    const int64_t words = (int64_t)X * Y * bv_words(Z);
    return bv_align(sizeof(unsigned)) + bv_align((size_t)((words + TR_CHUNK - 1) / TR_CHUNK) * sizeof(int)) +
           bv_align((size_t)words * sizeof(int));
}
static size_t tr_assign_workspace_bytes(int X, int Y, int Z) { return 2 * ru3d_skeleton_workspace_bytes(X, Y, Z); }

extern "C" int ru3d_site_assign(const uint64_t* site_bits, const uint64_t* region_bits, const int32_t* index,
                                const int32_t* site_ids, int64_t n, int X, int Y, int Z, int32_t* labels, void* ws,
                                size_t ws_bytes, void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    BV_REQUIRE_SHAPE("site_assign");
    RU3D_REQUIRE(n >= 0 && n <= (int64_t)X * Y * Z, "site_assign: n = %lld sites in a volume of %lld voxels", (long long)n,
                 (long long)X * Y * Z);
    RU3D_REQUIRE(site_bits && index && labels && ws && (site_ids || !n), "site_assign: bad argument (null pointer)");
    const size_t need = tr_assign_workspace_bytes(X, Y, Z);
    RU3D_REQUIRE(ws_bytes >= need && tr_assign_carved_bytes(X, Y, Z) <= need,
                 "site_assign: workspace of %zu bytes, %zu needed", ws_bytes, need);
    hipStream_t st = as_stream(stream);
    const int W = bv_words(Z);
    const int64_t words = (int64_t)X * Y * W, voxels = (int64_t)X * Y * Z;
    const int chunks = (int)((words + TR_CHUNK - 1) / TR_CHUNK);
    unsigned* err = (unsigned*)ws;
    int* counts = (int*)((char*)ws + bv_align(sizeof(unsigned)));
    int* prefix = (int*)((char*)counts + bv_align((size_t)chunks * sizeof(int)));
    if (hipMemsetAsync(err, 0, sizeof(unsigned), st) != hipSuccess) return ru3d_check_launch("site_assign (memset)");
    hipLaunchKernelGGL(tr_count_kernel, dim3(chunks), dim3(TR_CHUNK), 0, st, (const tr_u64*)site_bits, words, W, bv_tail(Z),
                       counts);
    hipLaunchKernelGGL(tr_scan_kernel, dim3(1), dim3(BV_SCAN_THREADS), 0, st, counts, chunks, (long long)n, err);
    hipLaunchKernelGGL(tr_prefix_kernel, dim3(chunks), dim3(TR_CHUNK), 0, st, (const tr_u64*)site_bits, words, W, bv_tail(Z),
                       (const int*)counts, prefix);
    const int64_t cap = (int64_t)ru3d_get_cu_budget() * 8;
    int64_t blocks = (voxels + 255) / 256;
    blocks = blocks > cap ? cap : blocks;
    hipLaunchKernelGGL(tr_assign_kernel, dim3((unsigned)blocks), dim3(256), 0, st, (const tr_u64*)site_bits,
                       (const tr_u64*)region_bits, (const int*)index, (const int*)site_ids, (long long)n, Z, W, voxels,
                       (const int*)prefix, (int*)labels, err);
    if (int rc = ru3d_check_launch("site_assign")) return rc;
    return tr_read_errors("site_assign", err, st);
}

#define TR_TALLY_WORKSPACE 256             // the error word

extern "C" int ru3d_territory_tally(const int32_t* labels, int K, const uint8_t* other, int num_other,
                                    const uint64_t* region_bits, int X, int Y, int Z, int64_t* table, void* ws,
                                    size_t ws_bytes, void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    BV_REQUIRE_SHAPE("territory_tally");
    RU3D_REQUIRE(K >= 0 && K < (1 << 30), "territory_tally: K = %d (0 .. 2^30 - 1)", K);
    RU3D_REQUIRE(num_other >= 0 && num_other <= 255 && (other || !num_other),
                 "territory_tally: num_other = %d (0 .. 255, 0 without `other`)", num_other);
    RU3D_REQUIRE(labels && table && ws, "territory_tally: bad argument (null pointer)");
    RU3D_REQUIRE(ws_bytes >= TR_TALLY_WORKSPACE, "territory_tally: workspace of %zu bytes, %zu needed", ws_bytes,
                 (size_t)TR_TALLY_WORKSPACE);
    hipStream_t st = as_stream(stream);
    const int64_t cells = ((int64_t)K + 1) * (num_other + 1), voxels = (int64_t)X * Y * Z;
    unsigned* err = (unsigned*)ws;
    if (hipMemsetAsync(err, 0, sizeof(unsigned), st) != hipSuccess ||
        hipMemsetAsync(table, 0, (size_t)cells * sizeof(int64_t), st) != hipSuccess)
        return ru3d_check_launch("territory_tally (memset)");
    const int64_t cap = (int64_t)ru3d_get_cu_budget() * 8;
    int64_t blocks = (voxels + 255) / 256;
    blocks = blocks > cap ? cap : blocks;
    if (cells <= TR_LDS_CELLS)
        hipLaunchKernelGGL(tr_tally_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, st, (const int*)labels, K, other,
                           num_other, (const tr_u64*)region_bits, Z, bv_words(Z), voxels, (unsigned long long*)table, err);
    else
        hipLaunchKernelGGL(tr_tally_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, st, (const int*)labels, K, other,
                           num_other, (const tr_u64*)region_bits, Z, bv_words(Z), voxels, (unsigned long long*)table, err);
    if (int rc = ru3d_check_launch("territory_tally")) return rc;
    return tr_read_errors("territory_tally", err, st);
}
