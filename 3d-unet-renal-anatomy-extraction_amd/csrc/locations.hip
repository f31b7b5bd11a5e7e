// Per-case class-location index for foreground-oversampled patches (the recipe of nnU-Net's data loader: index the
// voxels of every class once per case, then centre a patch on one of them).  For a label volume [X, Y, Z] with values
// 0 .. 31: the number of voxels of each class, its box, and an evenly rank-strided subsample of its voxels' linear
// indices in raster order - bitvol.h's three-launch compaction, widened from one predicate to 32 classes.
//   loc_init_kernel      the boxes start at (INT_MAX, -1) per axis.
//   loc_count_kernel     a workgroup takes a tile of LOC_CHUNK voxels; counts[class][tile] and the boxes.  The lanes of a
//                        wave carry different classes, so a wave walks the classes it holds (loc_next_class): ballot the
//                        lanes of the first unserved lane's class, count them, retire them.  Lane c of a wave keeps the
//                        count and the box of class c in registers; the four waves meet in LDS, and the boxes leave
//                        with one integer atomicMin / atomicMax per workgroup, class and bound (any arrival order gives
//                        the same bits).
//   loc_scan_kernel      one workgroup per class: bv_scan_chunks over the class's row of tile counts, the total to
//                        counts[class], the box closed (exclusive high end, zeros for an absent class), and -1 into the
//                        slots of the class's row that no voxel will fill.
//   loc_scatter_kernel   a voxel's rank among its class is its tile's offset + the class's voxels in the tile's earlier
//                        trips + those in the earlier waves of this trip + the ballot rank inside the wave.  Rank g of n
//                        is slot j0 = ceil(g m / n) of m = min(n, max_per_class) iff j0 < m and floor(j0 n / m) == g:
//                        the inverse of "slot j holds rank floor(j n / m)".  n comes from counts[] in device memory.
// Integer arithmetic only; no atomic decides a position or a value: two runs give the same bits.
#include "common.h"
#include "bitvol.h"
#include <limits.h>

#define LOC_THREADS BV_CHUNK_THREADS
#define LOC_WAVES BV_CHUNK_WAVES
#define LOC_CHUNK 2048                       // voxels per workgroup: the tile of prepare.hip's masked sample
#define LOC_TRIPS (LOC_CHUNK / LOC_THREADS)
#define LOC_CLASSES RU3D_CLASS_INDEX_CLASSES
#define LOC_MAX_PER_CLASS RU3D_CLASS_INDEX_MAX_PER_CLASS

static_assert(LOC_CLASSES == 32, "lane c of a wave keeps class c: at most 64 classes, and the header says 32");

// the class of a voxel, -1 for a value that is indexed nowhere
__device__ __forceinline__ int loc_class(uint8_t v) { return v < LOC_CLASSES ? (int)v : -1; }
__device__ __forceinline__ int loc_class(int64_t v) { return (v >= 0 && v < LOC_CLASSES) ? (int)v : -1; }

// The next class of the wave's walk: *todo holds the lanes not served yet (wave-uniform; start with the ballot of
// cls >= 0, loop while it is not 0).  Returns the class of the first of them - the same value in every lane -, leaves the
// lanes that carry it in *same and retires them from *todo.  Every lane of the wave calls it.
__device__ __forceinline__ int loc_next_class(int cls, bv_u64* todo, bv_u64* same) {
    const int c = __builtin_amdgcn_readfirstlane(__shfl(cls, __ffsll(*todo) - 1, 64));
    *same = __ballot(cls == c);
    *todo &= ~*same;
    return c;
}

__device__ __forceinline__ int loc_wave_min(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ int loc_wave_max(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return v;
}

__global__ __launch_bounds__(LOC_CLASSES * 6) void loc_init_kernel(int* __restrict__ boxes) {
    boxes[threadIdx.x] = (threadIdx.x & 1) ? -1 : INT_MAX;
}

template <typename L>
__global__ __launch_bounds__(LOC_THREADS) void loc_count_kernel(const L* __restrict__ lab, int Y, int Z, int n, int tiles,
                                                                 int* __restrict__ tile_counts, int* __restrict__ boxes) {
    __shared__ int s_cnt[LOC_WAVES][LOC_CLASSES];
    __shared__ int s_box[LOC_WAVES][LOC_CLASSES][6];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t base = (int64_t)blockIdx.x * LOC_CHUNK;
    int cnt = 0;                                                           // lane c: class c in this wave's voxels
    int lo[3] = {INT_MAX, INT_MAX, INT_MAX}, hi[3] = {-1, -1, -1};
#pragma unroll 1
    for (int k = 0; k < LOC_TRIPS; k++) {
        const int64_t i = base + k * LOC_THREADS + threadIdx.x;
        const int cls = i < n ? loc_class(lab[i]) : -1;
        const int r = (int)i / Z, z = (int)i - r * Z, x = r / Y, y = r - x * Y;     // read only where i < n
        bv_u64 todo = __ballot(cls >= 0);
        while (todo) {
            bv_u64 same;
            const int c = loc_next_class(cls, &todo, &same);
            const bool in = cls == c;
            // the linear index grows with the lane, and x with it: the first and the last lane of the class hold its ends
            const int x0 = __shfl(x, __ffsll(same) - 1, 64), x1 = __shfl(x, 63 - __clzll(same), 64);
            const int y0 = loc_wave_min(in ? y : INT_MAX), y1 = loc_wave_max(in ? y : -1);
            const int z0 = loc_wave_min(in ? z : INT_MAX), z1 = loc_wave_max(in ? z : -1);
            if (lane == c) {
                cnt += __popcll(same);
                lo[0] = min(lo[0], x0), hi[0] = max(hi[0], x1);
                lo[1] = min(lo[1], y0), hi[1] = max(hi[1], y1);
                lo[2] = min(lo[2], z0), hi[2] = max(hi[2], z1);
            }
        }
    }
    if (lane < LOC_CLASSES) {
        s_cnt[wave][lane] = cnt;
#pragma unroll
        for (int a = 0; a < 3; a++) s_box[wave][lane][2 * a] = lo[a], s_box[wave][lane][2 * a + 1] = hi[a];
    }
    __syncthreads();
    if (threadIdx.x < LOC_CLASSES * 6) {
        const int c = threadIdx.x / 6, j = threadIdx.x - c * 6;
        const int total = s_cnt[0][c] + s_cnt[1][c] + s_cnt[2][c] + s_cnt[3][c];
        if (j == 0) tile_counts[(int64_t)c * tiles + blockIdx.x] = total;
        if (total > 0) {                                                   // one atomic per workgroup, class and bound
            int v = s_box[0][c][j];
            for (int w = 1; w < LOC_WAVES; w++) v = (j & 1) ? max(v, s_box[w][c][j]) : min(v, s_box[w][c][j]);
            if (j & 1) atomicMax(boxes + threadIdx.x, v);
            else atomicMin(boxes + threadIdx.x, v);
        }
    }
}

// grid: one workgroup per class
__global__ __launch_bounds__(BV_SCAN_THREADS) void loc_scan_kernel(int* __restrict__ tile_counts, int tiles, int max_per_class,
                                                                    long long* __restrict__ counts, int* __restrict__ boxes,
                                                                    int* __restrict__ locations) {
    __shared__ long long s_sum[BV_SCAN_THREADS];
    const int c = blockIdx.x;
    const long long total = bv_scan_chunks(tile_counts + (int64_t)c * tiles, tiles, s_sum);
    if (threadIdx.x == 0) counts[c] = total;
    if (threadIdx.x < 6) {
        int* b = boxes + c * 6 + threadIdx.x;
        if (total == 0) *b = 0;
        else if (threadIdx.x & 1) *b += 1;                                 // the high end leaves exclusive
    }
    const int m = (int)min(total, (long long)max_per_class);
    for (int j = m + (int)threadIdx.x; j < max_per_class; j += BV_SCAN_THREADS) locations[(int64_t)c * max_per_class + j] = -1;
}

template <typename L>
__global__ __launch_bounds__(LOC_THREADS) void loc_scatter_kernel(const L* __restrict__ lab, int n, int tiles,
                                                                   const int* __restrict__ offsets,
                                                                   const long long* __restrict__ counts, int max_per_class,
                                                                   int* __restrict__ locations) {
    __shared__ int s_trip[2][LOC_WAVES][LOC_CLASSES];                      // two sets: one barrier per trip
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t base = (int64_t)blockIdx.x * LOC_CHUNK;
    // lane c < 32 of every wave keeps class c: its voxels in the volume (fewer than 2^31) and the rank of the next one
    const int mine = lane & (LOC_CLASSES - 1);
    const int total = (int)counts[mine];
    int run = offsets[(int64_t)mine * tiles + blockIdx.x];
#pragma unroll 1
    for (int k = 0; k < LOC_TRIPS; k++) {
        const int64_t i = base + k * LOC_THREADS + threadIdx.x;
        const int cls = i < n ? loc_class(lab[i]) : -1;
        int in_wave = 0, of_wave = 0;                                      // this lane's rank among its class in the wave; lane c: class c in the wave
        bv_u64 todo = __ballot(cls >= 0);
        while (todo) {
            bv_u64 same;
            const int c = loc_next_class(cls, &todo, &same);
            if (cls == c) in_wave = __popcll(same & (((bv_u64)1 << lane) - 1));
            if (lane == c) of_wave = __popcll(same);
        }
        if (lane < LOC_CLASSES) s_trip[k & 1][wave][lane] = of_wave;
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < LOC_WAVES; w++) {
            const int v = s_trip[k & 1][w][mine];
            before += w < wave ? v : 0;
            all += v;
        }
        const int first = run + before;                                    // lane c: the rank of this wave's first voxel of class c
        run += all;
        const int src = cls & (LOC_CLASSES - 1);
        const int g = __shfl(first, src, 64) + in_wave, nc = __shfl(total, src, 64);
        if (cls >= 0) {
            int slot = g;                                                  // n <= max_per_class: the complete list
            bool member = true;
            if (nc > max_per_class) {
                const long long j0 = ((long long)g * max_per_class + nc - 1) / nc;
                member = j0 < max_per_class && (j0 * nc) / max_per_class == g;
                slot = (int)j0;
            }
            if (member) locations[(int64_t)cls * max_per_class + slot] = (int)i;
        }
    }
}

// ------------------------------------------------------------------------------------------------ entry points
static inline int loc_tiles(int64_t n) { return (int)((n + LOC_CHUNK - 1) / LOC_CHUNK); }

extern "C" size_t ru3d_class_index_workspace_bytes(int X, int Y, int Z) {
    if (!bv_shape_ok(X, Y, Z)) return 0;
    return bv_align((size_t)LOC_CLASSES * loc_tiles((int64_t)X * Y * Z) * sizeof(int));
}

extern "C" int ru3d_class_index(const void* label, int label_dtype, int X, int Y, int Z, int max_per_class, int64_t* counts,
                                int32_t* boxes, int32_t* locations, void* ws, size_t ws_bytes, void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    RU3D_REQUIRE(bv_shape_ok(X, Y, Z), "class_index: volume %d x %d x %d is not supported (every extent >= 1, fewer than 2^31 "
                                       "voxels)", X, Y, Z);
    RU3D_REQUIRE(label_dtype == RU3D_LABEL_I64 || label_dtype == RU3D_LABEL_U8,
                 "class_index: label dtype code %d (RU3D_LABEL_I64 / RU3D_LABEL_U8)", label_dtype);
    RU3D_REQUIRE(max_per_class >= 1 && max_per_class <= LOC_MAX_PER_CLASS, "class_index: max_per_class %d (1 .. %d)",
                 max_per_class, LOC_MAX_PER_CLASS);
    RU3D_REQUIRE(label && counts && boxes && locations && ws, "class_index: bad argument (null pointer)");
    RU3D_REQUIRE(ws_bytes >= ru3d_class_index_workspace_bytes(X, Y, Z), "class_index: workspace of %zu bytes, %zu needed",
                 ws_bytes, ru3d_class_index_workspace_bytes(X, Y, Z));
    hipStream_t st = as_stream(stream);
    const int n = X * Y * Z, tiles = loc_tiles(n);
    int* tile_counts = (int*)ws;
    long long* totals = (long long*)counts;
    const dim3 grid(tiles), block(LOC_THREADS);
    hipLaunchKernelGGL(loc_init_kernel, dim3(1), dim3(LOC_CLASSES * 6), 0, st, boxes);
    if (label_dtype == RU3D_LABEL_U8)
        hipLaunchKernelGGL(loc_count_kernel<uint8_t>, grid, block, 0, st, (const uint8_t*)label, Y, Z, n, tiles, tile_counts,
                           boxes);
    else
        hipLaunchKernelGGL(loc_count_kernel<int64_t>, grid, block, 0, st, (const int64_t*)label, Y, Z, n, tiles, tile_counts,
                           boxes);
    hipLaunchKernelGGL(loc_scan_kernel, dim3(LOC_CLASSES), dim3(BV_SCAN_THREADS), 0, st, tile_counts, tiles, max_per_class,
                       totals, boxes, locations);
    if (label_dtype == RU3D_LABEL_U8)
        hipLaunchKernelGGL(loc_scatter_kernel<uint8_t>, grid, block, 0, st, (const uint8_t*)label, n, tiles,
                           (const int*)tile_counts, (const long long*)totals, max_per_class, locations);
    else
        hipLaunchKernelGGL(loc_scatter_kernel<int64_t>, grid, block, 0, st, (const int64_t*)label, n, tiles,
                           (const int*)tile_counts, (const long long*)totals, max_per_class, locations);
    return ru3d_check_launch("class_index");
}
