// Curve skeletons of packed masks: a topology-preserving 3D thinning and what is measured on its result (clDice counts,
// end and junction voxels, graph length, radius statistics).  The contract is written down in include/ru3d.h; the numpy
// twin that defines the result is transform._skeleton_numpy.
//
// Masks are the packed masks of bitvol.h, read with its bounded word fetch and z-neighbour view: the bits at z >= Z are
// 0, which is also what "outside the volume is background" needs along z.
//   sk_mark_kernel      candidates of a direction d: cand = m & ~shift(m, d), one word per lane.  +-x and +-y read the
//                       neighbouring row's word, +-z shift across the word boundary.
//   sk_subpass_kernel   one (direction, subfield) sub-pass, in place.  A workgroup owns 8 x 8 rows of the subfield's (x, y)
//                       parity by 4 words, one word per lane.  It first ORs its candidate words (masked to the subfield's
//                       z parity): all zero -> it leaves without touching the mask, which is what a late iteration costs.
//                       Otherwise it stages the 17 x 17 rows around its rows by 4 + 2 words in LDS (each word once from
//                       HBM), and every lane with candidates walks the set bits of its word: the 27-bit neighbourhood code
//                       from nine rows of three words, the two predicates by bit-mask flood fills inside the code
//                       (sk_simple), and one store of the word with the deleted bits cleared.  A lane owns its whole
//                       word: z and z + 2 share a word and a subfield, so nobody else writes it, and the words of the
//                       other rows this launch reads are only ever changed in bits of the same subfield, which are not
//                       26-adjacent to any candidate and are masked out of its code.  Every decision of a sub-pass is
//                       therefore taken on the mask as it was when the sub-pass began, whatever the launch geometry.
//   sk_classify_kernel  the number of set 26-neighbours of every voxel of a word at once: a bit-sliced counter (two bit
//                       planes and a saturation plane) fed with the 26 shifted neighbour words.  ends = count 1,
//                       junctions = count >= 3; the three totals go through integer atomics.
//   sk_pairs_kernel     pairs of 26-adjacent set voxels per half-space offset (13 integer totals), sk_length_kernel turns
//                       them into millimetres in a fixed order; sk_overlap_kernel the three popcounts of clDice.
//   sk_radius_kernel    (n, min, max, sum of square roots) of a vector of squared radii: one workgroup, lane t sums the
//                       elements t, t + 256, .. in order, then a halving tree - an order numpy restates.
// Integer atomics (vector memory operations) and fixed-order float64 sums only: the same bits in every run.
#include <math.h>
#include "common.h"
#include "bitvol.h"

#pragma clang fp contract(off)

typedef unsigned long long sk_u64;

// the 3 x 3 x 3 neighbourhood as a 27-bit code: bit 9 (dx + 1) + 3 (dy + 1) + (dz + 1), the voxel itself bit 13
#define SK_ALL 0x7ffffffu
#define SK_N26 0x7ffdfffu
#define SK_N18 0x2ebdebau
#define SK_N6 0x415410u
// cells a step along +z, -z, +y, -y may land on
#define SK_NZ0 0x6db6db6u
#define SK_NZ2 0x36db6dbu
#define SK_NY0 0x7e3f1f8u
#define SK_NY2 0xfc7e3fu

#define SK_TX 8                           // rows of the subfield along x per workgroup
#define SK_TY 8                           // rows along y
#define SK_TW 4                           // words per row: 8 * 8 * 4 = 256 lanes, one word each
#define SK_SX (2 * SK_TX + 1)             // staged rows along x: the subfield's rows and everything between and around
#define SK_SY (2 * SK_TY + 1)
#define SK_SW (SK_TW + 2)                 // staged words per row: one halo word on each side
#define SK_PITCH (SK_SW + 1)              // LDS row pitch in words, odd
#define SK_RTHREADS 256

__device__ __forceinline__ unsigned sk_grow26(unsigned r) {
    r |= ((r << 1) & SK_NZ0) | ((r >> 1) & SK_NZ2);
    r |= ((r << 3) & SK_NY0) | ((r >> 3) & SK_NY2);
    return (r | (r << 9) | (r >> 9)) & SK_ALL;
}
__device__ __forceinline__ unsigned sk_grow6(unsigned r) {
    return (r | ((r << 1) & SK_NZ0) | ((r >> 1) & SK_NZ2) | ((r << 3) & SK_NY0) | ((r >> 3) & SK_NY2) | (r << 9) | (r >> 9)) &
           SK_ALL;
}

// T26 = 1 and T6bar = 1 of the voxel whose neighbourhood code is `code`
__device__ __forceinline__ bool sk_simple(unsigned code) {
    const unsigned obj = code & SK_N26;
    if (!obj) return false;
    unsigned reach = obj & (0u - obj), grown;
    while ((grown = sk_grow26(reach) & obj) != reach) reach = grown;
    if (reach != obj) return false;
    const unsigned back = ~code & SK_N18, faces = back & SK_N6;
    if (!faces) return false;
    reach = faces & (0u - faces);
    while ((grown = sk_grow6(reach) & back) != reach) reach = grown;
    return (faces & ~reach) == 0;
}

// bits z - 1, z, z + 1 (z = 64 w + b) of the row whose words w - 1, w, w + 1 are prev, cur, next
__device__ __forceinline__ unsigned sk_three(sk_u64 prev, sk_u64 cur, sk_u64 next, int b) {
    unsigned t = b == 0 ? (unsigned)((cur << 1) | (prev >> 63)) : (unsigned)(cur >> (b - 1));
    if (b == 63) t |= (unsigned)(next & 1ull) << 2;
    return t & 7u;
}

// ------------------------------------------------------------------------------------------------ thinning
__global__ __launch_bounds__(256) void sk_mark_kernel(const sk_u64* __restrict__ mask, sk_u64* __restrict__ cand, int X, int Y,
                                                      int W, int d, int64_t words) {
    const int64_t xstep = (int64_t)Y * W;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < words; i += (int64_t)gridDim.x * 256) {
        const int64_t row = i / W;
        const int w = (int)(i - row * W), y = (int)(row % Y), x = (int)(row / Y);
        const sk_u64 m = mask[i];
        sk_u64 n = 0;                                                       // the neighbour at p + d, outside: background
        if (m) {
            switch (d) {
                case 0: n = x > 0 ? mask[i - xstep] : 0ull; break;
                case 1: n = x < X - 1 ? mask[i + xstep] : 0ull; break;
                case 2: n = y > 0 ? mask[i - W] : 0ull; break;
                case 3: n = y < Y - 1 ? mask[i + W] : 0ull; break;
                case 4: n = bv_zdown(w > 0 ? mask[i - 1] : 0ull, m); break;
                default: n = bv_zup(m, w < W - 1 ? mask[i + 1] : 0ull); break;
            }
        }
        cand[i] = m & ~n;
    }
}

__global__ __launch_bounds__(256) void sk_subpass_kernel(sk_u64* __restrict__ mask, const sk_u64* __restrict__ cand, int X, int Y,
                                                         int W, int sx, int sy, sk_u64 zsel, int YT, int WT,
                                                         unsigned long long* __restrict__ deleted) {
    __shared__ sk_u64 tile[SK_SX * SK_SY * SK_PITCH];
    int t = blockIdx.x;
    const int w0 = (t % WT) * SK_TW;
    t /= WT;
    const int y0 = sy + 2 * SK_TY * (t % YT), x0 = sx + 2 * SK_TX * (t / YT);      // the tile's first row of the subfield
    const int lw = threadIdx.x % SK_TW, ly = (threadIdx.x / SK_TW) % SK_TY, lx = threadIdx.x / (SK_TW * SK_TY);
    const int x = x0 + 2 * lx, y = y0 + 2 * ly, w = w0 + lw;
    const bool inside = x < X && y < Y && w < W;
    const int64_t at = ((int64_t)x * Y + y) * W + w;
    const sk_u64 c = inside ? cand[at] & zsel : 0ull;
    if (!__syncthreads_or(c != 0ull)) return;                               // nothing to decide here: the mask is not read

    for (int i = threadIdx.x; i < SK_SX * SK_SY * SK_SW; i += 256) {
        const int k = i % SK_SW, r = i / SK_SW;
        const int hx = r / SK_SY, hy = r - hx * SK_SY;
        tile[r * SK_PITCH + k] = bv_word(mask, X, Y, W, x0 - 1 + hx, y0 - 1 + hy, w0 - 1 + k);
    }
    __syncthreads();

    sk_u64 kill = 0;
    if (c) {
        sk_u64 rows[9][3];
#pragma unroll
        for (int r = 0; r < 9; r++) {
            const sk_u64* p = tile + ((2 * lx + r / 3) * SK_SY + (2 * ly + r % 3)) * SK_PITCH + lw;
#pragma unroll
            for (int k = 0; k < 3; k++) rows[r][k] = p[k];
        }
        sk_u64 todo = c & rows[4][1];
        while (todo) {                                                      // at most 32 trips: one per candidate
            const int b = __ffsll(todo) - 1;
            todo &= todo - 1;
            unsigned code = 0;
#pragma unroll
            for (int r = 0; r < 9; r++) code |= sk_three(rows[r][0], rows[r][1], rows[r][2], b) << (3 * r);
            if (__popc(code & SK_N26) != 1 && sk_simple(code)) kill |= 1ull << b;          // end voxels stay
        }
        if (kill) mask[at] = rows[4][1] & ~kill;
    }
    const int n = bv_wave_sum(__popcll(kill));
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(deleted, (unsigned long long)n);
}

// ------------------------------------------------------------------------------------------------ classification
__global__ __launch_bounds__(256) void sk_classify_kernel(const sk_u64* __restrict__ mask, sk_u64* __restrict__ ends,
                                                          sk_u64* __restrict__ junctions, int X, int Y, int W, int64_t words,
                                                          unsigned long long* __restrict__ counts) {
    int nv = 0, ne = 0, nj = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < words; i += (int64_t)gridDim.x * 256) {
        const int64_t row = i / W;
        const int w = (int)(i - row * W), y = (int)(row % Y), x = (int)(row / Y);
        const sk_u64 m = mask[i];
        sk_u64 e = 0, j = 0;
        if (m) {
            sk_u64 c0 = 0, c1 = 0, sat = 0;                                 // per voxel: count = c1 c0, or "4 or more"
#pragma unroll
            for (int r = 0; r < 9; r++) {
                const int nx = x + r / 3 - 1, ny = y + r % 3 - 1;
                const sk_u64 prev = bv_word(mask, X, Y, W, nx, ny, w - 1), cur = bv_word(mask, X, Y, W, nx, ny, w),
                             next = bv_word(mask, X, Y, W, nx, ny, w + 1);
#pragma unroll
                for (int dz = -1; dz <= 1; dz++) {
                    if (r == 4 && dz == 0) continue;
                    const sk_u64 v = bv_zview(prev, cur, next, dz);
                    const sk_u64 carry = c0 & v;
                    c0 ^= v;
                    sat |= c1 & carry;
                    c1 ^= carry;
                }
            }
            e = m & c0 & ~c1 & ~sat;
            j = m & ((c0 & c1) | sat);
        }
        ends[i] = e;
        junctions[i] = j;
        nv += __popcll(m);
        ne += __popcll(e);
        nj += __popcll(j);
    }
    nv = bv_wave_sum(nv), ne = bv_wave_sum(ne), nj = bv_wave_sum(nj);
    if ((threadIdx.x & 63) == 0) {
        if (nv) atomicAdd(&counts[0], (unsigned long long)nv);
        if (ne) atomicAdd(&counts[1], (unsigned long long)ne);
        if (nj) atomicAdd(&counts[2], (unsigned long long)nj);
    }
}

// ------------------------------------------------------------------------------------------------ length
struct sk_steps {
    double mm[13];
};

__global__ __launch_bounds__(256) void sk_pairs_kernel(const sk_u64* __restrict__ mask, int X, int Y, int W, int64_t words,
                                                       unsigned long long* __restrict__ pairs) {
    int n[13];
#pragma unroll
    for (int k = 0; k < 13; k++) n[k] = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < words; i += (int64_t)gridDim.x * 256) {
        const int64_t row = i / W;
        const int w = (int)(i - row * W), y = (int)(row % Y), x = (int)(row / Y);
        const sk_u64 m = mask[i];
        if (!m) continue;
#pragma unroll
        for (int r = 4; r < 9; r++) {                                       // the rows (0, 0), (0, 1), (1, -1), (1, 0), (1, 1)
            const int nx = x + r / 3 - 1, ny = y + r % 3 - 1;
            const sk_u64 prev = bv_word(mask, X, Y, W, nx, ny, w - 1), cur = r == 4 ? m : bv_word(mask, X, Y, W, nx, ny, w),
                         next = bv_word(mask, X, Y, W, nx, ny, w + 1);
#pragma unroll
            for (int dz = -1; dz <= 1; dz++) {
                const int cell = 3 * r + dz + 1;
                if (cell > 13) n[cell - 14] += __popcll(m & bv_zview(prev, cur, next, dz));
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 13; k++) {
        const int v = bv_wave_sum(n[k]);
        if ((threadIdx.x & 63) == 0 && v) atomicAdd(&pairs[k], (unsigned long long)v);
    }
}

__global__ void sk_length_kernel(const unsigned long long* __restrict__ pairs, const sk_steps steps, double* __restrict__ out) {
    if (threadIdx.x || blockIdx.x) return;
    double total = 0.0;
    for (int k = 0; k < 13; k++) total = total + (double)pairs[k] * steps.mm[k];
    out[0] = total;
}

// ------------------------------------------------------------------------------------------------ overlap
__global__ __launch_bounds__(256) void sk_overlap_kernel(const sk_u64* __restrict__ a, const sk_u64* __restrict__ b, int64_t words,
                                                         unsigned long long* __restrict__ counts) {
    int na = 0, nb = 0, nab = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < words; i += (int64_t)gridDim.x * 256) {
        const sk_u64 va = a[i], vb = b[i];
        na += __popcll(va);
        nb += __popcll(vb);
        nab += __popcll(va & vb);
    }
    na = bv_wave_sum(na), nb = bv_wave_sum(nb), nab = bv_wave_sum(nab);
    if ((threadIdx.x & 63) == 0) {
        if (na) atomicAdd(&counts[0], (unsigned long long)na);
        if (nb) atomicAdd(&counts[1], (unsigned long long)nb);
        if (nab) atomicAdd(&counts[2], (unsigned long long)nab);
    }
}

// ------------------------------------------------------------------------------------------------ radius statistics
__global__ __launch_bounds__(SK_RTHREADS) void sk_radius_kernel(const double* __restrict__ sq, long long n,
                                                                double* __restrict__ out) {
    __shared__ double s_min[SK_RTHREADS], s_max[SK_RTHREADS], s_sum[SK_RTHREADS];
    double mn = INFINITY, mx = 0.0, sum = 0.0;
    for (long long i = threadIdx.x; i < n; i += SK_RTHREADS) {
        const double v = sq[i];
        mn = fmin(mn, v);
        mx = fmax(mx, v);
        sum = sum + sqrt(v);
    }
    s_min[threadIdx.x] = mn;
    s_max[threadIdx.x] = mx;
    s_sum[threadIdx.x] = sum;
    __syncthreads();
    for (int h = SK_RTHREADS / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) {
            s_min[threadIdx.x] = fmin(s_min[threadIdx.x], s_min[threadIdx.x + h]);
            s_max[threadIdx.x] = fmax(s_max[threadIdx.x], s_max[threadIdx.x + h]);
            s_sum[threadIdx.x] = s_sum[threadIdx.x] + s_sum[threadIdx.x + h];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out[0] = (double)n;
        out[1] = s_min[0];
        out[2] = s_max[0];
        out[3] = s_sum[0];
    }
}

// ------------------------------------------------------------------------------------------------ host side
static inline unsigned sk_blocks(int64_t words) {
    const int64_t cap = (int64_t)ru3d_get_cu_budget() * 8;
    int64_t blocks = (words + 255) / 256;
    blocks = blocks > cap ? cap : blocks;
    return (unsigned)(blocks < 1 ? 1 : blocks);
}

#define SK_COUNTERS 256                   // bytes of integer counters at the head of the workspace

extern "C" size_t ru3d_skeleton_workspace_bytes(int X, int Y, int Z) {
    if (!bv_shape_ok(X, Y, Z)) return 0;
    return SK_COUNTERS + bv_align((size_t)X * Y * bv_words(Z) * sizeof(sk_u64));
}

extern "C" int ru3d_skeleton_thin(uint64_t* mask, int X, int Y, int Z, int max_iterations, void* ws, size_t ws_bytes,
                                  void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    BV_REQUIRE_SHAPE("skeleton_thin");
    RU3D_REQUIRE(mask && ws, "skeleton_thin: bad argument (null pointer)");
    RU3D_REQUIRE(ws_bytes >= ru3d_skeleton_workspace_bytes(X, Y, Z), "skeleton_thin: workspace of %zu bytes, %zu needed",
                 ws_bytes, ru3d_skeleton_workspace_bytes(X, Y, Z));
    hipStream_t st = as_stream(stream);
    const int W = bv_words(Z);
    const int64_t words = (int64_t)X * Y * W;
    unsigned long long* deleted = (unsigned long long*)ws;
    sk_u64* cand = (sk_u64*)((char*)ws + SK_COUNTERS);
    const int WT = (W + SK_TW - 1) / SK_TW;
    int iterations = 0;
    while (max_iterations < 0 || iterations < max_iterations) {
        if (hipMemsetAsync(deleted, 0, sizeof(unsigned long long), st) != hipSuccess)
            return ru3d_fail(-1, "skeleton_thin: clearing the deletion counter failed");
        for (int d = 0; d < 6; d++) {
            hipLaunchKernelGGL(sk_mark_kernel, dim3(sk_blocks(words)), dim3(256), 0, st, (const sk_u64*)mask, cand, X, Y, W, d,
                               words);
            for (int s = 0; s < 8; s++) {
                const int sx = s >> 2, sy = (s >> 1) & 1, sz = s & 1;
                if (sx >= X || sy >= Y || sz >= Z) continue;               // no voxel of this parity
                const int XT = ((X - sx + 1) / 2 + SK_TX - 1) / SK_TX, YT = ((Y - sy + 1) / 2 + SK_TY - 1) / SK_TY;
                const int64_t tiles = (int64_t)XT * YT * WT;
                RU3D_REQUIRE(tiles < ((int64_t)1 << 31), "skeleton_thin: %lld tiles", (long long)tiles);
                hipLaunchKernelGGL(sk_subpass_kernel, dim3((unsigned)tiles), dim3(256), 0, st, (sk_u64*)mask,
                                   (const sk_u64*)cand, X, Y, W, sx, sy, sz ? 0xaaaaaaaaaaaaaaaaull : 0x5555555555555555ull, YT,
                                   WT, deleted);
            }
        }
        if (ru3d_check_launch("skeleton_thin")) return -1;
        unsigned long long n = 0;                                           // the one host read of an iteration
        if (hipMemcpyAsync(&n, deleted, sizeof(n), hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess) {
            ru3d_check_launch("skeleton_thin (read back)");
            return ru3d_fail(-1, "skeleton_thin: reading the deletion counter back failed");
        }
        iterations++;
        if (!n) break;
    }
    return iterations;
}

extern "C" int ru3d_skeleton_classify(const uint64_t* skel, int X, int Y, int Z, uint64_t* ends, uint64_t* junctions,
                                      int64_t* counts, void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    BV_REQUIRE_SHAPE("skeleton_classify");
    RU3D_REQUIRE(skel && ends && junctions && counts, "skeleton_classify: bad argument (null pointer)");
    RU3D_REQUIRE(skel != ends && skel != junctions && ends != junctions, "skeleton_classify: the three masks must be distinct");
    hipStream_t st = as_stream(stream);
    const int W = bv_words(Z);
    const int64_t words = (int64_t)X * Y * W;
    if (hipMemsetAsync(counts, 0, 3 * sizeof(int64_t), st) != hipSuccess) return ru3d_check_launch("skeleton_classify (memset)");
    hipLaunchKernelGGL(sk_classify_kernel, dim3(sk_blocks(words)), dim3(256), 0, st, (const sk_u64*)skel, (sk_u64*)ends,
                       (sk_u64*)junctions, X, Y, W, words, (unsigned long long*)counts);
    return ru3d_check_launch("skeleton_classify");
}

extern "C" int ru3d_skeleton_length(const uint64_t* skel, int X, int Y, int Z, const double* spacing, double* out, void* ws,
                                    size_t ws_bytes, void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    BV_REQUIRE_SHAPE("skeleton_length");
    RU3D_REQUIRE(skel && spacing && out && ws, "skeleton_length: bad argument (null pointer)");
    RU3D_REQUIRE(ws_bytes >= SK_COUNTERS, "skeleton_length: workspace of %zu bytes, %d needed", ws_bytes, SK_COUNTERS);
    for (int a = 0; a < 3; a++)
        RU3D_REQUIRE(isfinite(spacing[a]) && spacing[a] > 0.0, "skeleton_length: spacing[%d] = %g (finite and > 0)", a,
                     spacing[a]);
    sk_steps steps;
    for (int k = 0; k < 13; k++) {
        const int cell = 14 + k;
        const double ax = spacing[0] * (cell / 9 - 1), ay = spacing[1] * ((cell / 3) % 3 - 1), az = spacing[2] * (cell % 3 - 1);
        const double a = ax * ax, b = ay * ay, c = az * az, bc = b + c;
        steps.mm[k] = sqrt(a + bc);
    }
    hipStream_t st = as_stream(stream);
    const int W = bv_words(Z);
    const int64_t words = (int64_t)X * Y * W;
    unsigned long long* pairs = (unsigned long long*)ws;
    if (hipMemsetAsync(pairs, 0, 13 * sizeof(unsigned long long), st) != hipSuccess)
        return ru3d_check_launch("skeleton_length (memset)");
    hipLaunchKernelGGL(sk_pairs_kernel, dim3(sk_blocks(words)), dim3(256), 0, st, (const sk_u64*)skel, X, Y, W, words, pairs);
    hipLaunchKernelGGL(sk_length_kernel, dim3(1), dim3(64), 0, st, (const unsigned long long*)pairs, steps, out);
    return ru3d_check_launch("skeleton_length");
}

extern "C" int ru3d_skeleton_overlap(const uint64_t* a, const uint64_t* b, int X, int Y, int Z, int64_t* counts, void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    BV_REQUIRE_SHAPE("skeleton_overlap");
    RU3D_REQUIRE(a && b && counts, "skeleton_overlap: bad argument (null pointer)");
    hipStream_t st = as_stream(stream);
    const int64_t words = (int64_t)X * Y * bv_words(Z);
    if (hipMemsetAsync(counts, 0, 3 * sizeof(int64_t), st) != hipSuccess) return ru3d_check_launch("skeleton_overlap (memset)");
    hipLaunchKernelGGL(sk_overlap_kernel, dim3(sk_blocks(words)), dim3(256), 0, st, (const sk_u64*)a, (const sk_u64*)b, words,
                       (unsigned long long*)counts);
    return ru3d_check_launch("skeleton_overlap");
}

extern "C" int ru3d_skeleton_radius_stats(const double* sq, int64_t n, double* out, void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    RU3D_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "skeleton_radius_stats: %lld values (0 .. 2^31 - 1)", (long long)n);
    RU3D_REQUIRE(out && (sq || n == 0), "skeleton_radius_stats: bad argument (null pointer)");
    hipLaunchKernelGGL(sk_radius_kernel, dim3(1), dim3(SK_RTHREADS), 0, as_stream(stream), sq, (long long)n, out);
    return ru3d_check_launch("skeleton_radius_stats");
}
