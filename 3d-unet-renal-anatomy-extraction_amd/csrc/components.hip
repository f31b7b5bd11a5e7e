// Connected-component labelling of a uint8 [X, Y, Z] volume (6-connectivity = scipy.ndimage.label's default structure)
// and the merge of the cascade (reference transform.py:5-11, data.py:464-492, trainer.py:203-240).
//
// Labelling is a union-find whose parent array IS the caller's `labels` buffer: -1 on background, the linear index of
// a parent on foreground, parent <= child always, so a component's root is its smallest linear index and the result is
// a pure function of the mask whatever the order of the atomics.
//   1. cc_local_kernel     one workgroup per 8 x 8 x 64 tile (z = lane): the z-runs come from a wave ballot, the y / x
//                          unions are atomicMin on a tile-local parent array in LDS; every voxel leaves with its tile
//                          root, and one 64-bit word per (x, y, z-tile) row marks which voxels are tile roots.
//   2. cc_seam_kernel      one thread per voxel on a tile face: unite it with its neighbour across the face.
//   3. cc_flatten_roots    tile roots only: L[r] = find(r).  Everything else still points at its tile root, so
//   4. cc_flatten_count    L[i] = find(i) is at most two hops; the same pass counts the roots of each 2048-voxel chunk.
//   5. cc_scan_kernel      the scan of the chunk counts (bitvol.h, as the sums of 4. and the ranks of 6.), K -> the
//                          caller's device int.
//   6. cc_rank_kernel      roots in linear-index order get their number (stored as -(number) - 1 in place),
//   7. cc_finalize_kernel  every voxel reads its root's number.
// Inside a launch other workgroups change L.  Every loop here reads L with agent-scope relaxed atomic loads, decides only
// on what an atomicMin returned, and moves to a strictly smaller index or stops: a stale parent is still an ancestor, so
// a stale read costs a retry and never a wrong union, and no thread ever waits for another one.  Visibility between the
// steps comes from the kernel boundaries.  Integer atomics only: two runs give identical bytes.
//
// Statistics / filter / region accumulate / cascade merge are streaming passes; the statistics reduce per tile in an
// LDS table first and issue one global atomic per (tile, component).
#include "common.h"
#include "bitvol.h"
#include <limits.h>

#define CC_TX 8
#define CC_TY 8
#define CC_TZ 64
#define CC_ROWS (CC_TX * CC_TY)
#define CC_TILE (CC_ROWS * CC_TZ)
#define CC_CHUNK 2048                       // voxels (or components) per workgroup of the numbering passes
#define CC_HASH 256                         // per-tile statistics table (entries)
#define CC_PROBES 8
#define CC_MAX_CLASSES 8
#define CC_MAX_KEEP RU3D_KEEP_LARGEST_MAX   // the k of ru3d_keep_largest_components: one selection pass each

typedef unsigned long long cc_u64;

__device__ __forceinline__ int cc_load(const int* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void cc_store(int* p, int v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ------------------------------------------------------------------------------------------------ union-find
// Both finds walk only to strictly smaller, non-negative indices: they end after at most `a` steps on any memory contents.
__device__ __forceinline__ int cc_lds_find(const int* lab, int a) {
    for (;;) {
        const int p = __hip_atomic_load(lab + a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (p < 0 || p >= a) return a;
        a = p;
    }
}
__device__ __forceinline__ void cc_lds_unite(int* lab, int a, int b) {
    for (;;) {
        a = cc_lds_find(lab, a);
        b = cc_lds_find(lab, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = atomicMin(&lab[a], b);      // a was a root when this returns a: it now hangs under b
        if (old >= a) return;
        a = old;                                    // a had a parent already: that parent and b are still to be united
    }
}
__device__ __forceinline__ int cc_find(const int* L, int a) {
    for (;;) {
        const int p = cc_load(L + a);
        if (p < 0 || p >= a) return a;
        a = p;
    }
}
__device__ __forceinline__ void cc_unite(int* L, int a, int b) {
    for (;;) {
        a = cc_find(L, a);
        b = cc_find(L, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = atomicMin(&L[a], b);
        if (old >= a) return;
        a = old;
    }
}

// ------------------------------------------------------------------------------------------------ 1. tile-local pass
__global__ __launch_bounds__(256) void cc_local_kernel(const uint8_t* __restrict__ mask, int X, int Y, int Z, int YT,
                                                       int ZT, int* __restrict__ L, cc_u64* __restrict__ rootbits) {
    __shared__ int lab[CC_TILE];
    __shared__ cc_u64 rows[CC_ROWS];
    const int tile = blockIdx.x;
    const int zt = tile % ZT;
    const int rt = tile / ZT;
    const int x0 = (rt / YT) * CC_TX, y0 = (rt % YT) * CC_TY, z0 = zt * CC_TZ;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int z = z0 + lane;

    for (int k = 0; k < CC_ROWS / 4; k++) {
        const int row = wave * (CC_ROWS / 4) + k;               // row = lx * 8 + ly
        const int x = x0 + (row >> 3), y = y0 + (row & 7);
        bool fg = false;
        if (x < X && y < Y && z < Z) fg = mask[((int64_t)x * Y + y) * Z + z] != 0;
        const cc_u64 m = __ballot(fg);
        const cc_u64 zeros_below = ~m & ((1ull << lane) - 1ull);
        const int start = zeros_below ? 64 - __clzll(zeros_below) : 0;      // first voxel of this lane's z-run
        lab[row * CC_TZ + lane] = fg ? row * CC_TZ + start : -1;
        if (lane == 0) rows[row] = m;
    }
    __syncthreads();

    // y and x neighbours: one union per stretch of z where both rows are foreground (the z-runs are united already)
    for (int k = 0; k < CC_ROWS / 4; k++) {
        const int row = wave * (CC_ROWS / 4) + k;
        const cc_u64 m = rows[row];
        if (row & 7) {
            cc_u64 b = m & rows[row - 1];
            b &= ~(b << 1);
            if ((b >> lane) & 1ull) cc_lds_unite(lab, row * CC_TZ + lane, (row - 1) * CC_TZ + lane);
        }
        if (row >> 3) {
            cc_u64 b = m & rows[row - CC_TY];
            b &= ~(b << 1);
            if ((b >> lane) & 1ull) cc_lds_unite(lab, row * CC_TZ + lane, (row - CC_TY) * CC_TZ + lane);
        }
    }
    __syncthreads();

    for (int k = 0; k < CC_ROWS / 4; k++) {
        const int row = wave * (CC_ROWS / 4) + k;
        const int t = row * CC_TZ + lane;
        const int x = x0 + (row >> 3), y = y0 + (row & 7);
        const bool fg = (rows[row] >> lane) & 1ull;
        int root = -1;
        if (fg) root = cc_lds_find(lab, t);
        const cc_u64 rb = __ballot(fg && root == t);
        if (x < X && y < Y) {
            const int64_t rowbase = ((int64_t)x * Y + y);
            if (z < Z) {
                int g = -1;
                if (fg) {
                    const int rr = root >> 6;
                    g = (int)(((int64_t)(x0 + (rr >> 3)) * Y + (y0 + (rr & 7))) * Z + (z0 + (root & 63)));
                }
                L[rowbase * Z + z] = g;
            }
            if (lane == 0) rootbits[rowbase * ZT + zt] = rb;
        }
    }
}

// ------------------------------------------------------------------------------------------------ 2. seams
// nx / ny / nz: number of voxels on the lower x / y / z faces of all tiles but the first along that axis.
__global__ __launch_bounds__(256) void cc_seam_kernel(int* __restrict__ L, int X, int Y, int Z, int YT, int ZT,
                                                      int64_t nx, int64_t ny, int64_t nz) {
    const int64_t total = nx + ny + nz;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        int x, y, z;
        int64_t step;
        bool run_check;                                     // the voxel below in z shares this voxel's two tiles
        if (i < nx) {
            z = (int)(i % Z);
            const int64_t r = i / Z;
            y = (int)(r % Y);
            x = ((int)(r / Y) + 1) * CC_TX;
            step = (int64_t)Y * Z;
            run_check = (z & (CC_TZ - 1)) != 0;
        } else if (i < nx + ny) {
            const int64_t j = i - nx;
            z = (int)(j % Z);
            const int64_t r = j / Z;
            y = ((int)(r % (YT - 1)) + 1) * CC_TY;
            x = (int)(r / (YT - 1));
            step = Z;
            run_check = (z & (CC_TZ - 1)) != 0;
        } else {
            const int64_t j = i - nx - ny;
            z = ((int)(j % (ZT - 1)) + 1) * CC_TZ;
            const int64_t r = j / (ZT - 1);
            y = (int)(r % Y);
            x = (int)(r / Y);
            step = 1;
            run_check = false;
        }
        if (x >= X || y >= Y || z >= Z) continue;           // cannot happen for consistent nx / ny / nz
        const int64_t g = ((int64_t)x * Y + y) * Z + z;
        const int64_t nb = g - step;
        if (cc_load(L + g) < 0 || cc_load(L + nb) < 0) continue;
        // both voxels one step down in z are foreground too: their tiles united them with these two, and that pair is
        // another thread's union
        if (run_check && cc_load(L + g - 1) >= 0 && cc_load(L + nb - 1) >= 0) continue;
        cc_unite(L, (int)g, (int)nb);
    }
}

// ------------------------------------------------------------------------------------------------ 3./4. flatten
__global__ __launch_bounds__(256) void cc_flatten_roots_kernel(int* __restrict__ L, const cc_u64* __restrict__ rootbits,
                                                               int Z, int ZT, int64_t words) {
    const int lane = threadIdx.x & 63;
    for (int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); w < words; w += (int64_t)gridDim.x * 4) {
        const cc_u64 bits = rootbits[w];
        if (!((bits >> lane) & 1ull)) continue;
        const int z = (int)(w % ZT) * CC_TZ + lane;
        if (z >= Z) continue;
        const int64_t g = (w / ZT) * Z + z;
        const int r = cc_find(L, (int)g);
        if (r != (int)g) cc_store(L + g, r);
    }
}

__global__ __launch_bounds__(256) void cc_flatten_count_kernel(int* __restrict__ L, int64_t n, int* __restrict__ counts) {
    const int64_t base = (int64_t)blockIdx.x * CC_CHUNK;
    int roots = 0;                                           // of this lane's eight voxels
    for (int k = 0; k < CC_CHUNK / 256; k++) {
        const int64_t i = base + k * 256 + threadIdx.x;
        if (i < n) {
            const int v = cc_load(L + i);
            if (v == (int)i) {
                roots++;
            } else if (v >= 0) {
                const int r = cc_find(L, v);
                if (r != v) cc_store(L + i, r);
            }
        }
    }
    bv_chunk_sum(roots, counts);
}

// ------------------------------------------------------------------------------------------------ 5. scan
// bv_scan_chunks over the chunk counts, the grand total -> *total_out
__global__ __launch_bounds__(BV_SCAN_THREADS) void cc_scan_kernel(int* __restrict__ counts, int n, int* __restrict__ total_out) {
    __shared__ int s_sum[BV_SCAN_THREADS];
    const int sum = bv_scan_chunks(counts, n, s_sum);
    if (threadIdx.x == BV_SCAN_THREADS - 1) *total_out = sum;
}

// ------------------------------------------------------------------------------------------------ 6. rank
// The chunk's flagged elements in index order get offsets[chunk] + 1, + 2, ...
// ROOTS: flagged = L[i] == i, the number is stored over the root as -(number) - 1.
// KEEP:  flagged = sizes[i] >= threshold, remap[i] = number, 0 for the others.
enum { CC_RANK_ROOTS = 0, CC_RANK_KEEP = 1 };
template <int MODE>
__global__ __launch_bounds__(256) void cc_rank_kernel(int* __restrict__ L, const int* __restrict__ sizes, int threshold,
                                                      int64_t n, const int* __restrict__ offsets) {
    __shared__ int s_part[BV_CHUNK_WAVES];
    const int64_t base = (int64_t)blockIdx.x * CC_CHUNK;
    int run = offsets[blockIdx.x];
    for (int k = 0; k < CC_CHUNK / 256; k++) {
        const int64_t i = base + k * 256 + threadIdx.x;
        bool flag = false;
        if (i < n) flag = MODE == CC_RANK_ROOTS ? (L[i] == (int)i) : (sizes[i] >= threshold);
        int slab;
        const int before = bv_ballot_rank(flag, s_part, &slab);
        __syncthreads();                                     // s_part is written again in the next trip
        if (i < n) {
            const int number = run + before + 1;
            if (MODE == CC_RANK_ROOTS) {
                if (flag) L[i] = -number - 1;
            } else {
                L[i] = flag ? number : 0;
            }
        }
        run += slab;
    }
}

// ------------------------------------------------------------------------------------------------ 7. finalize
// -1 -> 0; a numbered root -> its number; everything else holds its root's index and reads the number there (the root's
// own thread may have rewritten it to the plain number already: both spellings decode to the same value).
__global__ __launch_bounds__(256) void cc_finalize_kernel(int* __restrict__ L, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int v = cc_load(L + i);
        int out;
        if (v == -1) {
            out = 0;
        } else if (v < -1) {
            out = -v - 1;
        } else {
            const int e = cc_load(L + v);
            out = e < 0 ? -e - 1 : e;
        }
        cc_store(L + i, out);
    }
}

// keep[k] = sizes[k] >= threshold, counted per chunk
__global__ __launch_bounds__(256) void cc_keep_count_kernel(const int* __restrict__ sizes, int threshold, int64_t n,
                                                            int* __restrict__ counts) {
    const int64_t base = (int64_t)blockIdx.x * CC_CHUNK;
    int kept = 0;
    for (int k = 0; k < CC_CHUNK / 256; k++) {
        const int64_t i = base + k * 256 + threadIdx.x;
        kept += (i < n && sizes[i] >= threshold) ? 1 : 0;
    }
    bv_chunk_sum(kept, counts);
}

// The renumbering table of "keep the k largest": remap[i] = 1 .. kept in index order for the k largest of
// sizes[0 .. count), 0 for the others; among equal sizes the smaller index wins (np.argsort(-sizes, kind='stable')[:k]).
// *kept = min(k, count).  One workgroup and k selection passes over the table, in which remap marks what is picked.
__global__ __launch_bounds__(BV_SCAN_THREADS) void cc_pick_largest_kernel(const int* __restrict__ sizes, int count, int k,
                                                                          int* remap, int* kept) {
    __shared__ cc_u64 s_best[BV_SCAN_THREADS / RU3D_WAVE];
    __shared__ int s_pick[CC_MAX_KEEP];
    for (int i = threadIdx.x; i < count; i += BV_SCAN_THREADS) remap[i] = k >= count ? i + 1 : 0;
    if (k >= count) {                                        // everything stays, under its old number
        if (threadIdx.x == 0) *kept = count;
        return;
    }
    __syncthreads();
    for (int pass = 0; pass < k; pass++) {
        cc_u64 best = 0;                                     // (size, ~index): the maximum is the largest, first one
        for (int i = threadIdx.x; i < count; i += BV_SCAN_THREADS) {
            if (remap[i]) continue;
            const cc_u64 key = (cc_u64)(unsigned)max(sizes[i], 0) << 32 | (0xffffffffu - (unsigned)i);
            best = key > best ? key : best;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const cc_u64 other = bv_shfl_xor(best, o);
            best = other > best ? other : best;
        }
        if ((threadIdx.x & 63) == 0) s_best[threadIdx.x >> 6] = best;
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int w = 1; w < BV_SCAN_THREADS / RU3D_WAVE; w++) best = s_best[w] > best ? s_best[w] : best;
            const int pick = (int)(0xffffffffu - (unsigned)best);       // k < count: every pass finds one
            s_pick[pass] = pick;
            remap[pick] = 1;
        }
        __syncthreads();                                     // the pick is visible to the next pass, s_best is free
    }
    if (threadIdx.x == 0) {
        for (int a = 0; a < k; a++) {                        // the picks get their numbers in index order
            int number = 1;
            for (int b = 0; b < k; b++) number += s_pick[b] < s_pick[a] ? 1 : 0;
            remap[s_pick[a]] = number;
        }
        *kept = k;
    }
}

__global__ __launch_bounds__(256) void cc_filter_apply_kernel(const int* __restrict__ labels, int64_t n, int count,
                                                              const int* __restrict__ remap, uint8_t* mask,
                                                              int* labels_out) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int l = labels[i];
        const int nl = (l > 0 && l <= count) ? remap[l - 1] : 0;
        if (mask && nl == 0 && mask[i]) mask[i] = 0;
        if (labels_out) labels_out[i] = nl;
    }
}

// ------------------------------------------------------------------------------------------------ statistics
__global__ __launch_bounds__(256) void cc_stats_init_kernel(int* __restrict__ sizes, int* __restrict__ boxes, int count) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < count; i += gridDim.x * 256) {
        sizes[i] = 0;
#pragma unroll
        for (int a = 0; a < 3; a++) {
            boxes[(int64_t)i * 6 + 2 * a] = INT_MAX;
            boxes[(int64_t)i * 6 + 2 * a + 1] = 0;
        }
    }
}

__device__ __forceinline__ void cc_stats_add(int* size, int* box, int len, int x0, int x1, int y0, int y1, int z0, int z1) {
    atomicAdd(size, len);
    atomicMin(box + 0, x0);
    atomicMax(box + 1, x1);
    atomicMin(box + 2, y0);
    atomicMax(box + 3, y1);
    atomicMin(box + 4, z0);
    atomicMax(box + 5, z1);
}

// One workgroup per 8 x 8 x 64 tile.  The leader lane of every z-run adds the run to the tile's table in LDS (open
// addressing, CC_PROBES tries, then straight to global memory); the table is flushed with one set of atomics per entry.
__global__ __launch_bounds__(256) void cc_stats_kernel(const int* __restrict__ labels, int X, int Y, int Z, int YT, int ZT,
                                                       int count, int* __restrict__ sizes, int* __restrict__ boxes) {
    __shared__ int hkey[CC_HASH];
    __shared__ int hsize[CC_HASH];
    __shared__ int hbox[CC_HASH * 6];
    hkey[threadIdx.x] = 0;
    hsize[threadIdx.x] = 0;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        hbox[threadIdx.x * 6 + 2 * a] = INT_MAX;
        hbox[threadIdx.x * 6 + 2 * a + 1] = 0;
    }
    __syncthreads();
    const int tile = blockIdx.x;
    const int zt = tile % ZT;
    const int rt = tile / ZT;
    const int x0 = (rt / YT) * CC_TX, y0 = (rt % YT) * CC_TY, z0 = zt * CC_TZ;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int z = z0 + lane;
    for (int k = 0; k < CC_ROWS / 4; k++) {
        const int row = wave * (CC_ROWS / 4) + k;
        const int x = x0 + (row >> 3), y = y0 + (row & 7);
        int lab = 0;
        if (x < X && y < Y && z < Z) lab = labels[((int64_t)x * Y + y) * Z + z];
        const int prev = __shfl_up(lab, 1, 64);
        const bool first = lane == 0 || prev != lab;          // first voxel of a run of equal labels
        const cc_u64 starts = __ballot(first);
        const cc_u64 above = lane == 63 ? 0ull : starts >> (lane + 1);
        const int len = above ? __ffsll((long long)above) : 64 - lane;
        if (!first || lab <= 0 || lab > count) continue;
        const unsigned h = ((unsigned)lab * 2654435761u) >> 24;
        int slot = -1;
        for (int p = 0; p < CC_PROBES; p++) {
            const int s = (int)((h + p) & (CC_HASH - 1));
            const int old = atomicCAS(&hkey[s], 0, lab);
            if (old == 0 || old == lab) {
                slot = s;
                break;
            }
        }
        if (slot >= 0)
            cc_stats_add(&hsize[slot], &hbox[slot * 6], len, x, x + 1, y, y + 1, z, z + len);
        else
            cc_stats_add(&sizes[lab - 1], &boxes[(int64_t)(lab - 1) * 6], len, x, x + 1, y, y + 1, z, z + len);
    }
    __syncthreads();
    const int key = hkey[threadIdx.x];
    if (key > 0) {
        const int* b = &hbox[threadIdx.x * 6];
        cc_stats_add(&sizes[key - 1], &boxes[(int64_t)(key - 1) * 6], hsize[threadIdx.x], b[0], b[1], b[2], b[3], b[4], b[5]);
    }
}

// ------------------------------------------------------------------------------------------------ cascade merge
// total[target] += prob[inside], hits[target] += 1 (trainer.py:224-233): the region box starts at (bx, by, bz) in volume
// coordinates and is clipped to [tx0, tx0+sx) x ... here.  One thread per (voxel, class) element.
__global__ __launch_bounds__(256) void cc_region_accumulate_kernel(const float* __restrict__ prob, int ry, int rz, int C,
                                                                   int bx, int by, int bz, double* __restrict__ total,
                                                                   int* __restrict__ hits, int Y, int Z, int tx0, int ty0,
                                                                   int tz0, int sx, int sy, int sz) {
    const int64_t n = (int64_t)sx * sy * sz * C;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int c = (int)(i % C);
        int64_t r = i / C;
        const int z = tz0 + (int)(r % sz);
        r /= sz;
        const int y = ty0 + (int)(r % sy);
        const int x = tx0 + (int)(r / sy);
        const int64_t o = ((int64_t)x * Y + y) * Z + z;
        const int64_t s = ((int64_t)(x - bx) * ry + (y - by)) * rz + (z - bz);
        total[o * C + c] += (double)prob[s * C + c];
        if (c == 0) hits[o] += 1;
    }
}

// total / hits where hits > 0, then round (C == 1, half to even like np.around) or argmax_c softmax_c with the first
// maximum winning (trainer.py:235-240), in float64 like the host arithmetic.  A row that holds a NaN gives 0: np.argmax
// returns the first NaN of the all-NaN softmax row, and NaN -> uint8 is 0.
template <int C>
__global__ __launch_bounds__(256) void cc_cascade_merge_kernel(const double* __restrict__ total, const int* __restrict__ hits,
                                                               int64_t n, uint8_t* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int h = hits[i];
        double v[C];
        bool nan = false;
#pragma unroll
        for (int c = 0; c < C; c++) {
            v[c] = total[i * C + c];
            if (h > 0) v[c] = v[c] / (double)h;
            nan |= v[c] != v[c];
        }
        if (nan) {
            out[i] = 0;
            continue;
        }
        if (C == 1) {
            const double r = rint(v[0]);
            out[i] = (uint8_t)(int)fmin(fmax(r, 0.0), 255.0);
            continue;
        }
        double m = v[0];
#pragma unroll
        for (int c = 1; c < C; c++) m = fmax(m, v[c]);
        double e[C];
        double se = 0.0;
#pragma unroll
        for (int c = 0; c < C; c++) {
            e[c] = exp(v[c] - m);
            se += e[c];
        }
        int best = 0;
        double bv = e[0] / se;
#pragma unroll
        for (int c = 1; c < C; c++) {
            const double p = e[c] / se;
            if (p > bv) {
                bv = p;
                best = c;
            }
        }
        out[i] = (uint8_t)best;
    }
}

// ------------------------------------------------------------------------------------------------ host side
static inline int cc_div_up(int a, int b) { return (a + b - 1) / b; }
static inline int cc_stream_blocks(int64_t n) {
    int64_t b = (n + 255) / 256;
    return (int)(b > 16384 ? 16384 : (b < 1 ? 1 : b));
}
static inline size_t cc_rootbits_bytes(int X, int Y, int Z) {
    return bv_align((size_t)X * Y * cc_div_up(Z, CC_TZ) * sizeof(cc_u64));
}
static inline int64_t cc_chunks(int64_t n) { return (n + CC_CHUNK - 1) / CC_CHUNK; }

extern "C" size_t ru3d_components_workspace_bytes(int X, int Y, int Z) {
    if (!bv_shape_ok(X, Y, Z)) return 0;
    return cc_rootbits_bytes(X, Y, Z) + bv_align((size_t)cc_chunks((int64_t)X * Y * Z) * sizeof(int));
}

extern "C" int ru3d_label_components(const uint8_t* mask, int X, int Y, int Z, int32_t* labels, int32_t* count_dev,
                                     void* ws, size_t ws_bytes, void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    BV_REQUIRE_SHAPE("label_components");
    RU3D_REQUIRE(mask && labels && count_dev && ws, "label_components: bad argument (null pointer)");
    RU3D_REQUIRE(ws_bytes >= ru3d_components_workspace_bytes(X, Y, Z), "label_components: workspace of %zu bytes, %zu needed",
                 ws_bytes, ru3d_components_workspace_bytes(X, Y, Z));
    hipStream_t st = as_stream(stream);
    const int64_t n = (int64_t)X * Y * Z;
    const int XT = cc_div_up(X, CC_TX), YT = cc_div_up(Y, CC_TY), ZT = cc_div_up(Z, CC_TZ);
    const int64_t tiles = (int64_t)XT * YT * ZT;
    RU3D_REQUIRE(tiles < ((int64_t)1 << 31), "label_components: %lld tiles", (long long)tiles);
    cc_u64* rootbits = (cc_u64*)ws;
    int* counts = (int*)((char*)ws + cc_rootbits_bytes(X, Y, Z));
    const int chunks = (int)cc_chunks(n);
    int* L = labels;

    hipLaunchKernelGGL(cc_local_kernel, dim3((unsigned)tiles), dim3(256), 0, st, mask, X, Y, Z, YT, ZT, L, rootbits);
    const int64_t nx = (int64_t)(XT - 1) * Y * Z, ny = (int64_t)X * (YT - 1) * Z, nz = (int64_t)X * Y * (ZT - 1);
    if (nx + ny + nz > 0)
        hipLaunchKernelGGL(cc_seam_kernel, dim3(cc_stream_blocks(nx + ny + nz)), dim3(256), 0, st, L, X, Y, Z, YT, ZT, nx,
                           ny, nz);
    const int64_t words = (int64_t)X * Y * ZT;
    hipLaunchKernelGGL(cc_flatten_roots_kernel, dim3(cc_stream_blocks(words * 64)), dim3(256), 0, st, L, rootbits, Z, ZT,
                       words);
    hipLaunchKernelGGL(cc_flatten_count_kernel, dim3(chunks), dim3(256), 0, st, L, n, counts);
    hipLaunchKernelGGL(cc_scan_kernel, dim3(1), dim3(BV_SCAN_THREADS), 0, st, counts, chunks, count_dev);
    hipLaunchKernelGGL((cc_rank_kernel<CC_RANK_ROOTS>), dim3(chunks), dim3(256), 0, st, L, (const int*)nullptr, 0, n,
                       counts);
    hipLaunchKernelGGL(cc_finalize_kernel, dim3(cc_stream_blocks(n)), dim3(256), 0, st, L, n);
    return ru3d_check_launch("label_components");
}

extern "C" int ru3d_component_stats(const int32_t* labels, int X, int Y, int Z, int count, int32_t* sizes, int32_t* boxes,
                                    void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    BV_REQUIRE_SHAPE("component_stats");
    RU3D_REQUIRE(count >= 0, "component_stats: count %d", count);
    if (count == 0) return 0;
    RU3D_REQUIRE(labels && sizes && boxes, "component_stats: bad argument (null pointer)");
    hipStream_t st = as_stream(stream);
    const int XT = cc_div_up(X, CC_TX), YT = cc_div_up(Y, CC_TY), ZT = cc_div_up(Z, CC_TZ);
    const int64_t tiles = (int64_t)XT * YT * ZT;
    RU3D_REQUIRE(tiles < ((int64_t)1 << 31), "component_stats: %lld tiles", (long long)tiles);
    hipLaunchKernelGGL(cc_stats_init_kernel, dim3(cc_stream_blocks(count)), dim3(256), 0, st, sizes, boxes, count);
    hipLaunchKernelGGL(cc_stats_kernel, dim3((unsigned)tiles), dim3(256), 0, st, labels, X, Y, Z, YT, ZT, count, sizes,
                       boxes);
    return ru3d_check_launch("component_stats");
}

extern "C" size_t ru3d_filter_components_workspace_bytes(int count) {
    if (count <= 0) return 0;
    return bv_align((size_t)count * sizeof(int)) + bv_align((size_t)cc_chunks(count) * sizeof(int));
}

// The pass that ru3d_filter_components and ru3d_keep_largest_components share: remap[k] (made on `st` by the caller,
// count > 0) is the new number of component k + 1, 0 to drop it.  Without a component nothing is removed or kept.
static int cc_filter_apply(const char* what, const int32_t* labels, int64_t n, int count, const int* remap,
                           uint8_t* mask_inout, int32_t* labels_out, int32_t* kept_dev, hipStream_t st) {
    if (count == 0) {
        if (hipMemsetAsync(kept_dev, 0, sizeof(int), st) != hipSuccess) return ru3d_check_launch(what);
        if (labels_out && labels_out != labels)
            hipLaunchKernelGGL(cc_filter_apply_kernel, dim3(cc_stream_blocks(n)), dim3(256), 0, st, labels, n, 0,
                               (const int*)nullptr, (uint8_t*)nullptr, labels_out);
        return ru3d_check_launch(what);
    }
    hipLaunchKernelGGL(cc_filter_apply_kernel, dim3(cc_stream_blocks(n)), dim3(256), 0, st, labels, n, count, remap,
                       mask_inout, labels_out);
    return ru3d_check_launch(what);
}

extern "C" int ru3d_filter_components(const int32_t* labels, int X, int Y, int Z, int count, const int32_t* sizes,
                                      int threshold, uint8_t* mask_inout, int32_t* labels_out, int32_t* kept_dev, void* ws,
                                      size_t ws_bytes, void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    BV_REQUIRE_SHAPE("filter_components");
    RU3D_REQUIRE(count >= 0, "filter_components: count %d", count);
    RU3D_REQUIRE(labels && kept_dev && (count == 0 || sizes), "filter_components: bad argument (null pointer)");
    RU3D_REQUIRE(mask_inout || labels_out, "filter_components: neither a mask nor a label output");
    RU3D_REQUIRE(count == 0 || (ws && ws_bytes >= ru3d_filter_components_workspace_bytes(count)),
                 "filter_components: workspace of %zu bytes, %zu needed", ws_bytes,
                 ru3d_filter_components_workspace_bytes(count));
    hipStream_t st = as_stream(stream);
    int* remap = (int*)ws;
    if (count > 0) {
        int* counts = (int*)((char*)ws + bv_align((size_t)count * sizeof(int)));
        const int chunks = (int)cc_chunks(count);
        hipLaunchKernelGGL(cc_keep_count_kernel, dim3(chunks), dim3(256), 0, st, sizes, threshold, (int64_t)count, counts);
        hipLaunchKernelGGL(cc_scan_kernel, dim3(1), dim3(BV_SCAN_THREADS), 0, st, counts, chunks, kept_dev);
        hipLaunchKernelGGL((cc_rank_kernel<CC_RANK_KEEP>), dim3(chunks), dim3(256), 0, st, remap, sizes, threshold,
                           (int64_t)count, counts);
    }
    return cc_filter_apply("filter_components", labels, (int64_t)X * Y * Z, count, remap, mask_inout, labels_out, kept_dev, st);
}

// the workspace is the one of ru3d_filter_components (its renumbering table; the chunk counts stay unused)
extern "C" int ru3d_keep_largest_components(const int32_t* labels, int X, int Y, int Z, int count, const int32_t* sizes, int k,
                                            uint8_t* mask_inout, int32_t* labels_out, int32_t* kept_dev, void* ws,
                                            size_t ws_bytes, void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    BV_REQUIRE_SHAPE("keep_largest_components");
    RU3D_REQUIRE(count >= 0, "keep_largest_components: count %d", count);
    RU3D_REQUIRE(k >= 1 && k <= CC_MAX_KEEP, "keep_largest_components: k = %d (1 .. %d)", k, CC_MAX_KEEP);
    RU3D_REQUIRE(labels && kept_dev && (count == 0 || sizes), "keep_largest_components: bad argument (null pointer)");
    RU3D_REQUIRE(mask_inout || labels_out, "keep_largest_components: neither a mask nor a label output");
    RU3D_REQUIRE(count == 0 || (ws && ws_bytes >= ru3d_filter_components_workspace_bytes(count)),
                 "keep_largest_components: workspace of %zu bytes, %zu needed", ws_bytes,
                 ru3d_filter_components_workspace_bytes(count));
    hipStream_t st = as_stream(stream);
    int* remap = (int*)ws;
    if (count > 0)
        hipLaunchKernelGGL(cc_pick_largest_kernel, dim3(1), dim3(BV_SCAN_THREADS), 0, st, sizes, count, k, remap, kept_dev);
    return cc_filter_apply("keep_largest_components", labels, (int64_t)X * Y * Z, count, remap, mask_inout, labels_out,
                           kept_dev, st);
}

extern "C" int ru3d_region_accumulate(const float* prob, int rx, int ry, int rz, int num_classes, int bx, int by, int bz,
                                      double* total, int32_t* hits, int X, int Y, int Z, void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    BV_REQUIRE_SHAPE("region_accumulate");
    RU3D_REQUIRE(prob && total && hits, "region_accumulate: bad argument (null pointer)");
    RU3D_REQUIRE(rx > 0 && ry > 0 && rz > 0, "region_accumulate: region of %dx%dx%d", rx, ry, rz);
    RU3D_REQUIRE(num_classes >= 1 && num_classes <= CC_MAX_CLASSES, "region_accumulate: %d classes (max %d)", num_classes,
                 CC_MAX_CLASSES);
    const int64_t ex = (int64_t)bx + rx, ey = (int64_t)by + ry, ez = (int64_t)bz + rz;
    const int tx0 = bx > 0 ? bx : 0, ty0 = by > 0 ? by : 0, tz0 = bz > 0 ? bz : 0;
    const int64_t sx = (ex < X ? ex : X) - tx0, sy = (ey < Y ? ey : Y) - ty0, sz = (ez < Z ? ez : Z) - tz0;
    if (sx <= 0 || sy <= 0 || sz <= 0) return 0;          // the box misses the volume: nothing to add
    const int64_t n = sx * sy * sz * num_classes;
    hipLaunchKernelGGL(cc_region_accumulate_kernel, dim3(cc_stream_blocks(n)), dim3(256), 0, as_stream(stream), prob, ry, rz,
                       num_classes, bx, by, bz, total, hits, Y, Z, tx0, ty0, tz0, (int)sx, (int)sy, (int)sz);
    return ru3d_check_launch("region_accumulate");
}

template <int C>
static int cc_merge_launch(const double* total, const int* hits, int64_t n, uint8_t* out, hipStream_t st) {
    hipLaunchKernelGGL((cc_cascade_merge_kernel<C>), dim3(cc_stream_blocks(n)), dim3(256), 0, st, total, hits, n, out);
    return ru3d_check_launch("cascade_merge");
}

extern "C" int ru3d_cascade_merge(const double* total, const int32_t* hits, int X, int Y, int Z, int num_classes,
                                  uint8_t* out, void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    BV_REQUIRE_SHAPE("cascade_merge");
    RU3D_REQUIRE(total && hits && out, "cascade_merge: bad argument (null pointer)");
    RU3D_REQUIRE(num_classes >= 1 && num_classes <= CC_MAX_CLASSES, "cascade_merge: %d classes (max %d)", num_classes,
                 CC_MAX_CLASSES);
    hipStream_t st = as_stream(stream);
    const int64_t n = (int64_t)X * Y * Z;
    switch (num_classes) {
        case 1: return cc_merge_launch<1>(total, hits, n, out, st);
        case 2: return cc_merge_launch<2>(total, hits, n, out, st);
        case 3: return cc_merge_launch<3>(total, hits, n, out, st);
        case 4: return cc_merge_launch<4>(total, hits, n, out, st);
        case 5: return cc_merge_launch<5>(total, hits, n, out, st);
        case 6: return cc_merge_launch<6>(total, hits, n, out, st);
        case 7: return cc_merge_launch<7>(total, hits, n, out, st);
        default: return cc_merge_launch<8>(total, hits, n, out, st);
    }
}
