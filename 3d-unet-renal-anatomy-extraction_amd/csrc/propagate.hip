// Geodesic propagation on bit-packed masks (bitvol.h): scipy.ndimage.binary_propagation, and with it binary_fill_holes,
// for volumes that stay in HBM.  reach = the seed plus every voxel of `allowed` that a chain of neighbours (the six face
// neighbours, or all 26 of the 3 x 3 x 3 cube) connects to a seed voxel or to the outside of the volume where that reads
// as set.  A seed voxel outside `allowed` stays set and spreads into its allowed neighbours, as in scipy's masked
// dilation.
//
// A fixpoint by rounds, one launch per round; no workgroup ever waits for another one.
//   tile      a workgroup owns PG_TX x PG_TY rows x PG_TW words (16 x 16 x 128 voxels), one thread per row.  The row's
//             words of `allowed` and `reach` live in registers; `reach` is mirrored in LDS with one halo row on each
//             x / y side and one halo word on each z side (only its nearest bit is used): 18 x 18 rows x 4 words.
//   outside   a voxel outside the volume reads as set when every axis along which it is outside has its bit in
//             border_axes, else as clear.  The bits at z >= Z are never allowed and are 0 in everything written.
//   inside    each trip ORs the neighbour rows' words (for the cube also their views from z - 1 and z + 1), the own
//             row's bv_zdown / bv_zup, ANDs with `allowed` and runs a log-step fill through the allowed bits of each
//             word, until __syncthreads_or says that no row changed.  A trip that goes on set a bit, so the loop ends
//             after at most PG_TILE_VOXELS trips.
//   back      only the words that changed are stored; thread 0 adds 1 to changed[round] when the tile changed: one
//             integer atomic per workgroup and round.
// Halo words are read from global `reach` while the neighbouring workgroups may be storing them in the same launch, so
// every access to `reach` is an agent-scope relaxed atomic (as cc_load in components.hip).  Bits are only ever set, and
// a set bit is always truly reachable: a stale read costs a round and never a wrong bit.  A round in which no tile
// changed read final halos everywhere and found every tile at its own fixpoint, so it is the global fixpoint.  That
// fixpoint is unique (the least set that holds the seed and is closed under "allowed neighbour of a member"), so two
// runs give identical bytes however the rounds interleave.  Rounds on a converged volume only read it.
//
// No floating point, no float atomics, no LDS beyond the static tile.  Convergence is the caller's loop: the entry point
// runs the rounds it is asked for and leaves the per-round counts of changed tiles in the caller's device buffer.
#include "common.h"
#include "bitvol.h"

#define PG_TX 16
#define PG_TY 16
#define PG_TW 2                              // words per row of a tile
#define PG_PX (PG_TX + 2)
#define PG_PY (PG_TY + 2)
#define PG_SW (PG_TW + 2)                    // staged words per row: one halo word on each z side
#define PG_PITCH (PG_SW + 1)                 // LDS row pitch in words, odd
#define PG_TILE_VOXELS (PG_TX * PG_TY * PG_TW * 64)
#define PG_MAX_ROUNDS 64

typedef bv_u64 pg_u64;

__device__ __forceinline__ pg_u64 pg_load(const pg_u64* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void pg_store(pg_u64* p, pg_u64 v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// g plus every bit that a run of set bits of p connects to a bit of g, upwards and downwards inside the word
__device__ __forceinline__ pg_u64 pg_fill(pg_u64 g, pg_u64 p) {
    pg_u64 up = g, pu = p, dn = g, pd = p;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        up |= pu & (up << s);
        pu &= pu << s;
        dn |= pd & (dn >> s);
        pd &= pd >> s;
    }
    return up | dn;
}

// word gw of row (gx, gy) of `reach` as the flood sees it: the stored word inside the volume, the border value outside
__device__ __forceinline__ pg_u64 pg_reach_word(const pg_u64* reach, int X, int Y, int W, pg_u64 tail, int border, int gx,
                                                int gy, int gw) {
    const bool in_x = (unsigned)gx < (unsigned)X, in_y = (unsigned)gy < (unsigned)Y, in_w = (unsigned)gw < (unsigned)W;
    const bool row_in = in_x && in_y;
    const pg_u64 row_out = ((in_x || (border & 1)) && (in_y || (border & 2))) ? ~0ull : 0ull;
    const pg_u64 zfill = (border & 4) ? (row_in ? ~0ull : row_out) : 0ull;       // the voxels at z < 0 and z >= Z
    if (!in_w) return zfill;
    const pg_u64 v = row_in ? pg_load(reach + ((int64_t)gx * Y + gy) * W + gw) : row_out;
    return gw == W - 1 ? (v & ~tail) | (zfill & tail) : v;
}

template <bool CUBE>
__global__ __launch_bounds__(256) void pg_round_kernel(const pg_u64* __restrict__ allowed, pg_u64 invert, pg_u64* reach, int X,
                                                       int Y, int Z, int W, int YT, int WT, int border, int* changed) {
    __shared__ pg_u64 s_reach[PG_PX * PG_PY * PG_PITCH];
    int t = blockIdx.x;
    const int w0 = (t % WT) * PG_TW;
    t /= WT;
    const int y0 = (t % YT) * PG_TY, x0 = (t / YT) * PG_TX;
    const pg_u64 tail = bv_tail(Z);

    for (int i = threadIdx.x; i < PG_PX * PG_PY * PG_SW; i += 256) {
        const int k = i % PG_SW, r = i / PG_SW;
        const int hx = r / PG_PY, hy = r - hx * PG_PY;
        const bool edge_x = hx == 0 || hx == PG_PX - 1, edge_y = hy == 0 || hy == PG_PY - 1, edge_w = k == 0 || k == PG_SW - 1;
        // the cross reads no edge or corner neighbour
        const bool used = CUBE || (int)edge_x + (int)edge_y + (int)edge_w <= 1;
        s_reach[r * PG_PITCH + k] = used ? pg_reach_word(reach, X, Y, W, tail, border, x0 - 1 + hx, y0 - 1 + hy, w0 - 1 + k)
                                         : 0ull;
    }

    const int lx = threadIdx.x / PG_TY, ly = threadIdx.x % PG_TY;
    const int x = x0 + lx, y = y0 + ly;
    const bool row_in = x < X && y < Y;
    pg_u64 a[PG_TW];
#pragma unroll
    for (int j = 0; j < PG_TW; j++)
        a[j] = row_in ? (bv_word_masked(allowed, X, Y, W, tail, x, y, w0 + j) ^ invert) & (w0 + j < W ? ~0ull : 0ull) &
                            (w0 + j == W - 1 ? ~tail : ~0ull)
                      : 0ull;
    __syncthreads();

    pg_u64* own = s_reach + ((lx + 1) * PG_PY + (ly + 1)) * PG_PITCH;
    pg_u64 first[PG_TW], cur[PG_TW];
#pragma unroll
    for (int j = 0; j < PG_TW; j++) first[j] = cur[j] = own[j + 1];

    for (int trip = 0; trip < PG_TILE_VOXELS; trip++) {
        pg_u64 next[PG_TW];
        {
            pg_u64 w[PG_SW];
#pragma unroll
            for (int k = 0; k < PG_SW; k++) w[k] = own[k];
#pragma unroll
            for (int j = 0; j < PG_TW; j++) next[j] = bv_zdown(w[j], w[j + 1]) | bv_zup(w[j + 1], w[j + 2]);
        }
        if (CUBE) {
#pragma unroll
            for (int n = 0; n < 9; n++) {
                if (n == 4) continue;
                const pg_u64* q = own + ((n / 3 - 1) * PG_PY + (n % 3 - 1)) * PG_PITCH;
                pg_u64 w[PG_SW];
#pragma unroll
                for (int k = 0; k < PG_SW; k++) w[k] = q[k];
#pragma unroll
                for (int j = 0; j < PG_TW; j++) next[j] |= w[j + 1] | bv_zdown(w[j], w[j + 1]) | bv_zup(w[j + 1], w[j + 2]);
            }
        } else {
#pragma unroll
            for (int j = 0; j < PG_TW; j++)
                next[j] |= own[j + 1 - PG_PY * PG_PITCH] | own[j + 1 + PG_PY * PG_PITCH] | own[j + 1 - PG_PITCH] |
                           own[j + 1 + PG_PITCH];
        }
        int grew = 0;
#pragma unroll
        for (int j = 0; j < PG_TW; j++) {
            next[j] = pg_fill(cur[j] | (next[j] & a[j]), a[j]);
            grew |= next[j] != cur[j];
        }
        if (!__syncthreads_or(grew)) break;                  // every row has read its neighbours
#pragma unroll
        for (int j = 0; j < PG_TW; j++) own[j + 1] = cur[j] = next[j];
        __syncthreads();
    }

    int wrote = 0;
    if (row_in) {
#pragma unroll
        for (int j = 0; j < PG_TW; j++) {
            if (w0 + j < W && cur[j] != first[j]) {
                pg_store(reach + ((int64_t)x * Y + y) * W + w0 + j, w0 + j == W - 1 ? cur[j] & ~tail : cur[j]);
                wrote = 1;
            }
        }
    }
    if (__syncthreads_or(wrote) && threadIdx.x == 0) atomicAdd(changed, 1);
}

// out = mask | ~reach inside the volume
__global__ __launch_bounds__(256) void pg_fill_result_kernel(const pg_u64* __restrict__ mask, const pg_u64* __restrict__ reach,
                                                             pg_u64* __restrict__ out, int W, pg_u64 tail, int64_t words) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < words; i += (int64_t)gridDim.x * 256) {
        const pg_u64 v = mask[i] | ~reach[i];
        out[i] = (int)(i % W) == W - 1 ? v & ~tail : v;
    }
}

// ------------------------------------------------------------------------------------------------ host side
extern "C" int ru3d_binary_propagate(const uint64_t* allowed, int invert_allowed, uint64_t* reach, int X, int Y, int Z,
                                     int connectivity, int border_axes, int rounds, int32_t* changed_dev, void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    BV_REQUIRE_SHAPE("binary_propagate");
    RU3D_REQUIRE(allowed && reach && changed_dev, "binary_propagate: bad argument (null pointer)");
    RU3D_REQUIRE(allowed != reach, "binary_propagate: allowed and reach are one buffer");
    RU3D_REQUIRE(invert_allowed == 0 || invert_allowed == 1, "binary_propagate: invert_allowed %d (0 or 1)", invert_allowed);
    RU3D_REQUIRE(connectivity == 1 || connectivity == 3, "binary_propagate: connectivity %d (1 = faces, 3 = the cube)",
                 connectivity);
    RU3D_REQUIRE(border_axes >= 0 && border_axes <= 7, "binary_propagate: border_axes %d (bits 0 .. 2)", border_axes);
    RU3D_REQUIRE(rounds >= 1 && rounds <= PG_MAX_ROUNDS, "binary_propagate: %d rounds (1 .. %d)", rounds, PG_MAX_ROUNDS);
    const int W = bv_words(Z);
    const int XT = (X + PG_TX - 1) / PG_TX, YT = (Y + PG_TY - 1) / PG_TY, WT = (W + PG_TW - 1) / PG_TW;
    const int64_t tiles = (int64_t)XT * YT * WT;
    RU3D_REQUIRE(tiles < ((int64_t)1 << 31), "binary_propagate: %lld tiles", (long long)tiles);
    hipStream_t st = as_stream(stream);
    if (hipMemsetAsync(changed_dev, 0, (size_t)rounds * sizeof(int32_t), st) != hipSuccess)
        return ru3d_check_launch("binary_propagate");
    const pg_u64 invert = invert_allowed ? ~0ull : 0ull;
    for (int r = 0; r < rounds; r++) {
        if (connectivity == 3)
            hipLaunchKernelGGL(pg_round_kernel<true>, dim3((unsigned)tiles), dim3(256), 0, st, (const pg_u64*)allowed, invert,
                               (pg_u64*)reach, X, Y, Z, W, YT, WT, border_axes, changed_dev + r);
        else
            hipLaunchKernelGGL(pg_round_kernel<false>, dim3((unsigned)tiles), dim3(256), 0, st, (const pg_u64*)allowed, invert,
                               (pg_u64*)reach, X, Y, Z, W, YT, WT, border_axes, changed_dev + r);
    }
    return ru3d_check_launch("binary_propagate");
}

extern "C" int ru3d_mask_fill_result(const uint64_t* mask, const uint64_t* reach, uint64_t* out, int X, int Y, int Z,
                                     void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    BV_REQUIRE_SHAPE("mask_fill_result");
    RU3D_REQUIRE(mask && reach && out, "mask_fill_result: bad argument (null pointer)");
    RU3D_REQUIRE(out != mask && out != reach, "mask_fill_result: not an in-place operation");
    const int W = bv_words(Z);
    const int64_t words = (int64_t)X * Y * W;
    const int64_t blocks = (words + 255) / 256;
    hipLaunchKernelGGL(pg_fill_result_kernel, dim3((unsigned)(blocks > 16384 ? 16384 : blocks)), dim3(256), 0,
                       as_stream(stream), (const pg_u64*)mask, (const pg_u64*)reach, (pg_u64*)out, W, bv_tail(Z), words);
    return ru3d_check_launch("mask_fill_result");
}
