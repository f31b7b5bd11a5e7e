// Local thickness of a bit-packed mask (Hildebrand and Rueegsegger 1997): per voxel the squared radius of the largest
// inscribed ball that contains it.  Packed masks and the count / scan / rank pieces of the candidate list are those of
// bitvol.h; the inscribed radii R2 come from ru3d_edt_squared of the complement (csrc/distance.hip).
//
// The contract (include/ru3d.h, "local thickness"): T2(x) = max { R2(p) : p in M, d2(x, p) < R2(p) } with
// d2 = fl(A + fl(B + C)), A = fl(fl(sx dx)^2), B and C alike, in float64 - the expression of ru3d_edt_squared, so this
// file too is compiled with floating-point contraction off.  It is a formula, not an algorithm: a scatter of balls
// with a maximum, and a maximum does not depend on the order of its operands.
//   th_count / th_scan / th_index   the linear indices of the mask's voxels in element order, bitvol.h's compaction over
//                      the word popcounts of 256-word chunks: every lane writes the voxels of its word at their ranks.
//   th_paint_kernel    one wavefront per candidate p, four per workgroup, grid-stride over the list.  The box of the ball
//                      is floor(sqrt(R2) / s) + 1 voxels to either side per axis, clipped to the volume: the + 1 absorbs
//                      any rounding of the square root and of the division, and the test with the contract's expression
//                      decides every voxel.  Lanes run along z, so the accesses of a row are contiguous; a box fewer than
//                      33 voxels long in z (a vessel's lumen) puts 64 / length rows of the box side by side in the wave.
//                      A row is skipped when fl(A + B) >= R2: C >= 0 and rounding is monotone, so
//                      fl(A + fl(B + C)) >= fl(A + B) for every voxel of the row.
//                      The update.  Nonnegative doubles and +inf order like their 64-bit patterns, so the maximum is an
//                      unsigned 64-bit atomicMax on the bits.  out[x] is read with a plain load first and the atomic is
//                      issued only when the candidate is larger.  out only ever grows while the kernel runs, so a stale
//                      read can only be too small: it costs one redundant atomic and never loses an update.  The final
//                      value of every voxel is the maximum of the same set of values whatever the order the waves ran
//                      in: the same bytes in every run, under every CU budget, sorted or not.
//                      With strict < a ball never reaches a clear voxel (R2(p) <= d2(p, b) for every clear b, and d2 is
//                      symmetric), so the paint needs no mask test and every voxel outside the mask keeps its 0.
//                      R2 = +inf (no clear voxel: the mask is the whole volume and every voxel a candidate) is handled
//                      before any box is computed: the candidate stores +inf at its own voxel.
//                      Work counters: the voxels tested with the contract's expression and the atomics issued, summed in
//                      registers and added once per wave.
#include <math.h>
#include "common.h"
#include "bitvol.h"

#pragma clang fp contract(off)

typedef unsigned long long th_u64;

#define TH_GCHUNK 256                     // words of a compaction chunk = threads of its workgroup
#define TH_THREADS 256                    // workgroup of the paint: four wavefronts, one candidate each
#define TH_WAVES (TH_THREADS / RU3D_WAVE)

// fl(fl(s d)^2)
__device__ __forceinline__ double th_sq(double s, int d) {
    const double t = s * (double)d;
    return t * t;
}

// ------------------------------------------------------------------------------------------------ candidate list
__device__ __forceinline__ th_u64 th_word(const th_u64* __restrict__ q, int64_t i, int64_t words, int W, th_u64 tail) {
    if (i >= words) return 0ull;
    return (i % W) == W - 1 ? q[i] & ~tail : q[i];
}

__global__ __launch_bounds__(TH_GCHUNK) void th_count_kernel(const th_u64* __restrict__ q, int64_t words, int W, th_u64 tail,
                                                             int* __restrict__ counts) {
    bv_chunk_sum(__popcll(th_word(q, (int64_t)blockIdx.x * TH_GCHUNK + threadIdx.x, words, W, tail)), counts);
}

__global__ __launch_bounds__(BV_SCAN_THREADS) void th_scan_kernel(int* __restrict__ counts, int chunks,
                                                                  long long* __restrict__ total) {
    __shared__ int s_sum[BV_SCAN_THREADS];
    const int sum = bv_scan_chunks(counts, chunks, s_sum);
    if (threadIdx.x == BV_SCAN_THREADS - 1) *total = (long long)sum;
}

__global__ __launch_bounds__(TH_GCHUNK) void th_index_kernel(const th_u64* __restrict__ q, int64_t words, int W, int Z,
                                                             th_u64 tail, const int* __restrict__ offsets,
                                                             int* __restrict__ index, long long capacity) {
    const int64_t i = (int64_t)blockIdx.x * TH_GCHUNK + threadIdx.x;
    th_u64 m = th_word(q, i, words, W, tail);
    long long rank = (long long)offsets[blockIdx.x] + bv_chunk_rank(__popcll(m));
    if (!m) return;
    const int64_t row = i / W;
    const int64_t base = row * Z + 64 * (int)(i - row * W);                 // < X*Y*Z < 2^31
    while (m) {                                                             // at most 64 trips: one per set bit
        const int b = __ffsll(m) - 1;
        m &= m - 1;
        if (rank < capacity) index[rank] = (int)(base + b);
        rank++;
    }
}

// ------------------------------------------------------------------------------------------------ paint
__global__ __launch_bounds__(TH_THREADS) void th_paint_kernel(const double* __restrict__ r2, const int* __restrict__ index,
                                                              long long n, int X, int Y, int Z, double sx, double sy,
                                                              double sz, th_u64* __restrict__ out,
                                                              th_u64* __restrict__ work) {
    const int lane = threadIdx.x & (RU3D_WAVE - 1);
    const long long stride = (long long)gridDim.x * TH_WAVES;
    const long long total = (long long)X * Y * Z;
    th_u64 tested = 0, issued = 0;
    for (long long i = (long long)blockIdx.x * TH_WAVES + (threadIdx.x >> 6); i < n; i += stride) {
        const int p = index[i];                                             // wave-uniform
        if (p < 0 || p >= total) continue;                                  // not a voxel: nothing is touched
        const double R = r2[p];
        const th_u64 Rbits = (th_u64)__double_as_longlong(R);
        if (!(R > 0.0)) continue;                                           // a clear voxel (or NaN) paints nothing
        if (R == INFINITY) {                                                // no clear voxel anywhere
            if (lane == 0) out[p] = Rbits;
            continue;
        }
        const int px = p / (Y * Z), py = (p - px * (Y * Z)) / Z, pz = p - (px * Y + py) * Z;
        const double r = sqrt(R);
        // half-extents: the quotient may be huge for a tiny spacing, so it is clipped as a double
        const double qx = floor(r / sx) + 1.0, qy = floor(r / sy) + 1.0, qz = floor(r / sz) + 1.0;
        const int hx = qx < (double)X ? (int)qx : X, hy = qy < (double)Y ? (int)qy : Y, hz = qz < (double)Z ? (int)qz : Z;
        const int x0 = max(px - hx, 0), x1 = min(px + hx, X - 1);
        const int y0 = max(py - hy, 0), y1 = min(py + hy, Y - 1);
        const int z0 = max(pz - hz, 0), z1 = min(pz + hz, Z - 1);
        const int ny = y1 - y0 + 1, zl = z1 - z0 + 1, rows = (x1 - x0 + 1) * ny;          // rows <= X*Y < 2^31
        // a short box puts g rows side by side: lane = rl * zl + zi
        const int g = zl >= RU3D_WAVE ? 1 : RU3D_WAVE / zl;
        const int rl = zl >= RU3D_WAVE ? 0 : lane / zl;
        const int zi0 = zl >= RU3D_WAVE ? lane : lane - rl * zl;
        if (rl >= g) continue;                                              // lanes beyond the last whole row of a trip
        for (int row = rl; row < rows; row += g) {
            const int ix = row / ny;
            const int x = x0 + ix, y = y0 + (row - ix * ny);
            const double A = th_sq(sx, x - px), B = th_sq(sy, y - py);
            if (A + B >= R) continue;                                       // every voxel of the row is at least that far
            th_u64* line = out + ((long long)x * Y + y) * Z;
            for (int zi = zi0; zi < zl; zi += RU3D_WAVE) {
                const int z = z0 + zi;
                const double d2 = A + (B + th_sq(sz, z - pz));
                tested++;
                if (d2 < R && line[z] < Rbits) {
                    atomicMax(line + z, Rbits);
                    issued++;
                }
            }
        }
    }
    if (work) {                                                             // once per wave, not once per lane
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            tested += __shfl_xor(tested, o, RU3D_WAVE);
            issued += __shfl_xor(issued, o, RU3D_WAVE);
        }
        if (lane == 0) {
            if (tested) atomicAdd(work, tested);
            if (issued) atomicAdd(work + 1, issued);
        }
    }
}

// ------------------------------------------------------------------------------------------------ host side
extern "C" size_t ru3d_thickness_workspace_bytes(int X, int Y, int Z) {
    if (!bv_shape_ok(X, Y, Z)) return 0;
    const int64_t words = (int64_t)X * Y * bv_words(Z);
    return bv_align((size_t)((words + TH_GCHUNK - 1) / TH_GCHUNK) * sizeof(int));
}

extern "C" int ru3d_thickness_candidates(const uint64_t* bits, int X, int Y, int Z, int32_t* index, int64_t capacity,
                                         int64_t* count, void* ws, size_t ws_bytes, void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    BV_REQUIRE_SHAPE("thickness_candidates");
    RU3D_REQUIRE(bits && count && ws, "thickness_candidates: bad argument (null pointer)");
    RU3D_REQUIRE(!index || capacity >= 1, "thickness_candidates: capacity %lld of the index list (>= 1)", (long long)capacity);
    RU3D_REQUIRE(((uintptr_t)ws & 7) == 0, "thickness_candidates: workspace at %p is not aligned to 8 bytes", ws);
    RU3D_REQUIRE(ws_bytes >= ru3d_thickness_workspace_bytes(X, Y, Z), "thickness_candidates: workspace of %zu bytes, %zu needed",
                 ws_bytes, ru3d_thickness_workspace_bytes(X, Y, Z));
    hipStream_t st = as_stream(stream);
    const int W = bv_words(Z);
    const int64_t words = (int64_t)X * Y * W;
    const int chunks = (int)((words + TH_GCHUNK - 1) / TH_GCHUNK);
    int* counts = (int*)ws;
    hipLaunchKernelGGL(th_count_kernel, dim3(chunks), dim3(TH_GCHUNK), 0, st, (const th_u64*)bits, words, W, bv_tail(Z), counts);
    hipLaunchKernelGGL(th_scan_kernel, dim3(1), dim3(BV_SCAN_THREADS), 0, st, counts, chunks, (long long*)count);
    if (index)
        hipLaunchKernelGGL(th_index_kernel, dim3(chunks), dim3(TH_GCHUNK), 0, st, (const th_u64*)bits, words, W, Z, bv_tail(Z),
                           (const int*)counts, (int*)index, (long long)capacity);
    return ru3d_check_launch("thickness_candidates");
}

extern "C" int ru3d_thickness_paint(const double* r2, const int32_t* index, int64_t n, int X, int Y, int Z,
                                    const double* spacing, double* out, int64_t* work_dev, void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    BV_REQUIRE_SHAPE("thickness_paint");
    RU3D_REQUIRE(n >= 0 && n <= (int64_t)X * Y * Z, "thickness_paint: %lld candidates in a volume of %lld voxels",
                 (long long)n, (long long)X * Y * Z);
    RU3D_REQUIRE(r2 && out && spacing && (index || n == 0), "thickness_paint: bad argument (null pointer)");
    RU3D_REQUIRE((const void*)r2 != (const void*)out, "thickness_paint: not an in-place operation (r2 == out)");
    for (int a = 0; a < 3; a++)
        RU3D_REQUIRE(isfinite(spacing[a]) && spacing[a] > 0.0, "thickness_paint: spacing[%d] = %g (finite and > 0)", a,
                     spacing[a]);
    hipStream_t st = as_stream(stream);
    if (hipMemsetAsync(out, 0, (size_t)X * Y * Z * sizeof(double), st) != hipSuccess)
        return ru3d_check_launch("thickness_paint (memset)");
    if (work_dev && hipMemsetAsync(work_dev, 0, 2 * sizeof(int64_t), st) != hipSuccess)
        return ru3d_check_launch("thickness_paint (memset)");
    if (n > 0) {
        const int64_t cap = (int64_t)ru3d_get_cu_budget() * 8, need = (n + TH_WAVES - 1) / TH_WAVES;
        hipLaunchKernelGGL(th_paint_kernel, dim3((unsigned)(need < cap ? need : cap)), dim3(TH_THREADS), 0, st, r2,
                           (const int*)index, (long long)n, X, Y, Z, spacing[0], spacing[1], spacing[2], (th_u64*)out,
                           (th_u64*)work_dev);
    }
    return ru3d_check_launch("thickness_paint");
}
