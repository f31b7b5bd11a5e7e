// Geodesic distance and nearest-seed labels inside a packed mask (bitvol.h): the weighted version of the flood of
// propagate.hip.  A multi-source shortest-path transform on the 6- or 26-neighbour voxel graph of `allowed` with INTEGER
// step lengths, for volumes that stay in HBM.  The contract is in include/ru3d.h, "geodesic distance"; in short:
//   key       one 64-bit word per voxel, dist << 32 | label; all ones = not reached.  A seed starts at key = label.
//   rule      for a voxel v of `allowed` and a reached neighbour u at offset k:  key[v] = min(key[v], key[u] + (w[k] << 32)),
//             admitted only when dist(u) + w[k] <= limit.
//   result    the least fixpoint of the rule.  Integer sums make (dist, label) strictly monotone under a step, so it is
//             the answer of a lexicographic Dijkstra - the smallest distance and, among the seeds at that distance, the
//             smallest label - whatever the order of the updates and however stale the reads.
//
// A fixpoint by rounds, one launch per round; no workgroup ever waits for another one.
//   tile      a workgroup owns GD_TX x GD_TY x GD_TZ voxels (8 x 8 x 32) and holds their keys with a one-voxel halo in
//             LDS, z fastest: 10 x 10 rows of 34 keys at a pitch of 35.  Thread t owns the column (x = 0 .. 7, y = t / 32,
//             z = t % 32): the 32 lanes of a half wave read 32 consecutive keys, which no pitch can make collide; the odd
//             pitch spreads the rows of the staging loop, whose lanes run across row ends.
//   allowed   the tile's half word per (x, y) row comes from the packed words (bv_word_masked), one bit per owned voxel
//             ends up in a register.  Bits outside the volume are never allowed, so nothing outside is ever written.
//   trips     each trip relaxes every owned allowed voxel from LDS into registers, __syncthreads_or tells whether any
//             key fell, the new keys go back to LDS.  The loop ends at the tile's own fixpoint or after GD_MAX_TRIPS
//             trips; a tile that stops at the cap has stored keys and so counts as changed.
//   back      only the keys that fell are stored; thread 0 adds 1 to changed[round] when the tile stored any and writes
//             the tile's byte of this round's activity map: one integer atomic per workgroup and round.
//   idle      two byte maps of tile activity alternate between the rounds.  A tile whose own and 26 neighbouring tiles
//             stored nothing in the previous round would read what it read before and exits on those flags (skip_idle);
//             the first round of a fresh run takes every tile as active.  A tile without an allowed voxel can store
//             nothing and exits after its allowed words.
// Halo keys are read from global memory while the neighbouring workgroups may be storing them in the same launch, so
// every access to `keys` is an agent-scope relaxed 64-bit atomic (as pg_load / pg_store).  A voxel has one owner, keys
// only ever fall, and every key ever stored is the length of a real path from the seed it names: a stale halo costs a
// round and never a wrong value.  A tile that read a stale halo has a neighbour that stored in that round and runs in
// the next, so a round in which no tile stored read final halos everywhere: the global fixpoint.
//
// No floating point, no float atomics, no 64-bit atomic minimum, no LDS beyond the static tile.  Convergence is the
// caller's loop: the entry point runs the rounds it is asked for and leaves the per-round counts of changed tiles in the
// caller's device buffer.
#include "common.h"
#include "bitvol.h"

#define GD_TX 8
#define GD_TY 8
#define GD_TZ 32
#define GD_PX (GD_TX + 2)
#define GD_PY (GD_TY + 2)
#define GD_SZ (GD_TZ + 2)                    // staged keys per row: one halo key on each z side
#define GD_PITCH (GD_SZ + 1)                 // LDS row pitch in keys, odd
#define GD_THREADS 256
#define GD_MAX_TRIPS RU3D_GEODESIC_MAX_TRIPS
#define GD_MAX_ROUNDS 64
#define GD_MAX_WEIGHT (1u << 20)
#define GD_UNLIMITED 0xFFFFFFFEu
#define GD_NONE (~0ull)

static_assert(GD_THREADS == GD_TY * GD_TZ, "a thread per (y, z) column of the tile");
static_assert(GD_TZ == 32, "a tile is half a packed word along z");

typedef bv_u64 gd_u64;

struct gd_weights {
    uint32_t w[26];                          // the offsets in ascending (dx, dy, dz) without the centre; 0: no such step
};

__device__ __forceinline__ gd_u64 gd_load(const gd_u64* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void gd_store(gd_u64* p, gd_u64 v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// best after the step from a neighbour with key n over a step of length w; refused: the step was turned down by the limit
__device__ __forceinline__ gd_u64 gd_relax(gd_u64 best, gd_u64 n, uint32_t w, uint32_t limit, int& refused) {
    if (n != GD_NONE) {
        if ((n >> 32) + w <= (gd_u64)limit) {
            const gd_u64 cand = n + ((gd_u64)w << 32);
            best = cand < best ? cand : best;
        } else {
            refused = 1;
        }
    }
    return best;
}

template <bool CUBE>
__global__ __launch_bounds__(GD_THREADS) void gd_round_kernel(const gd_u64* __restrict__ allowed, gd_u64 invert, gd_u64* keys,
                                                               int X, int Y, int Z, int XT, int YT, int ZT, gd_weights wt,
                                                               uint32_t limit, int all_active,
                                                               const uint8_t* __restrict__ active_prev,
                                                               uint8_t* __restrict__ active_next, int* changed, int* flags) {
    __shared__ gd_u64 s_key[GD_PX * GD_PY * GD_PITCH];
    __shared__ uint32_t s_allow[GD_TX * GD_TY];
    const int tile = blockIdx.x;
    const int tz = tile % ZT, ty = (tile / ZT) % YT, tx = tile / (ZT * YT);
    const int tid = threadIdx.x;

    if (!all_active) {                       // did this tile or one of its 26 neighbours store in the previous round?
        int busy = 0;
        if (tid < 27) {
            const int nx = tx + tid / 9 - 1, ny = ty + (tid / 3) % 3 - 1, nz = tz + tid % 3 - 1;
            if ((unsigned)nx < (unsigned)XT && (unsigned)ny < (unsigned)YT && (unsigned)nz < (unsigned)ZT)
                busy = active_prev[((int64_t)nx * YT + ny) * ZT + nz];
        }
        if (!__syncthreads_or(busy)) {
            if (tid == 0) active_next[tile] = 0;
            return;
        }
    }

    const int x0 = tx * GD_TX, y0 = ty * GD_TY, z0 = tz * GD_TZ;
    {                                        // the allowed bits of the tile: one half word per (x, y) row
        uint32_t bits = 0;
        if (tid < GD_TX * GD_TY) {
            const int x = x0 + tid / GD_TY, y = y0 + tid % GD_TY;
            if (x < X && y < Y) {
                const int W = bv_words(Z), wi = z0 >> 6;
                const gd_u64 tail = bv_tail(Z);
                const gd_u64 raw = allowed ? bv_word_masked(allowed, X, Y, W, tail, x, y, wi) ^ invert : ~0ull;
                bits = (uint32_t)((raw & (wi == W - 1 ? ~tail : ~0ull)) >> (z0 & 63));
            }
            s_allow[tid] = bits;
        }
        if (!__syncthreads_or(bits != 0)) {  // nothing in here may change
            if (tid == 0) active_next[tile] = 0;
            return;
        }
    }

    for (int i = tid; i < GD_PX * GD_PY * GD_SZ; i += GD_THREADS) {
        const int hz = i % GD_SZ, r = i / GD_SZ;
        const int hx = r / GD_PY, hy = r - hx * GD_PY;
        const int gx = x0 - 1 + hx, gy = y0 - 1 + hy, gz = z0 - 1 + hz;
        const bool edge_x = hx == 0 || hx == GD_PX - 1, edge_y = hy == 0 || hy == GD_PY - 1, edge_z = hz == 0 || hz == GD_SZ - 1;
        // the face steps read no edge or corner neighbour
        const bool used = CUBE || (int)edge_x + (int)edge_y + (int)edge_z <= 1;
        const bool in = (unsigned)gx < (unsigned)X && (unsigned)gy < (unsigned)Y && (unsigned)gz < (unsigned)Z;
        s_key[r * GD_PITCH + hz] = used && in ? gd_load(keys + ((int64_t)gx * Y + gy) * Z + gz) : GD_NONE;
    }
    __syncthreads();

    const int ly = tid / GD_TZ, lz = tid % GD_TZ;
    int mine = 0;                            // bit x: the owned voxel (x, ly, lz) is allowed
#pragma unroll
    for (int x = 0; x < GD_TX; x++) mine |= (int)((s_allow[x * GD_TY + ly] >> lz) & 1u) << x;
    gd_u64* own = s_key + (GD_PY + ly + 1) * GD_PITCH + lz + 1;               // the owned voxel of x = 0
    gd_u64 first[GD_TX], cur[GD_TX];
#pragma unroll
    for (int x = 0; x < GD_TX; x++) first[x] = cur[x] = own[x * GD_PY * GD_PITCH];

    int stuck = 0;                           // an owned allowed voxel is unreached and the limit turned a step to it down
    for (int trip = 0; trip < GD_MAX_TRIPS; trip++) {
        gd_u64 next[GD_TX];
        int fell = 0;
        stuck = 0;
#pragma unroll
        for (int x = 0; x < GD_TX; x++) {
            next[x] = cur[x];
            if (mine >> x & 1) {
                const gd_u64* c = own + x * GD_PY * GD_PITCH;
                gd_u64 best = cur[x];
                int refused = 0;
#pragma unroll
                for (int k = 0; k < 26; k++) {
                    const int o = k < 13 ? k : k + 1;                        // the centre is offset 13 of the 27
                    const int dx = o / 9 - 1, dy = (o / 3) % 3 - 1, dz = o % 3 - 1;
                    if (!CUBE && dx * dx + dy * dy + dz * dz != 1) continue;
                    if (wt.w[k] == 0) continue;
                    best = gd_relax(best, c[(dx * GD_PY + dy) * GD_PITCH + dz], wt.w[k], limit, refused);
                }
                fell |= best != cur[x];
                stuck |= refused && best == GD_NONE;
                next[x] = best;
            }
        }
        if (!__syncthreads_or(fell)) break;                  // every thread has read its neighbours
#pragma unroll
        for (int x = 0; x < GD_TX; x++) {
            if (next[x] != cur[x]) own[x * GD_PY * GD_PITCH] = cur[x] = next[x];
        }
        __syncthreads();
    }

    int wrote = 0;
#pragma unroll
    for (int x = 0; x < GD_TX; x++) {
        if (cur[x] != first[x]) {                            // only an allowed voxel, and so one inside the volume
            gd_store(keys + ((int64_t)(x0 + x) * Y + y0 + ly) * Z + z0 + lz, cur[x]);
            wrote = 1;
        }
    }
    if (stuck && limit == GD_UNLIMITED) flags[1] = 1;        // the caller confirms it at the fixpoint (include/ru3d.h)
    wrote = __syncthreads_or(wrote);
    if (tid == 0) {
        active_next[tile] = wrote ? 1 : 0;
        if (wrote) atomicAdd(changed, 1);
    }
}

// keys from seeds: label > 0 -> distance 0 with that label, 0 -> not reached; a negative value raises flags[0]
__global__ __launch_bounds__(256) void gd_init_kernel(const int32_t* __restrict__ seeds, gd_u64* __restrict__ keys, int64_t n,
                                                      int* flags) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int32_t s = seeds[i];
        keys[i] = s > 0 ? (gd_u64)s : GD_NONE;
        if (s < 0) flags[0] = 1;
    }
}

// dist = the high half (all ones where not reached), labels = the low half (0 where not reached)
__global__ __launch_bounds__(256) void gd_split_kernel(const gd_u64* __restrict__ keys, uint32_t* __restrict__ dist,
                                                       int32_t* __restrict__ labels, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const gd_u64 k = keys[i];
        dist[i] = (uint32_t)(k >> 32);
        labels[i] = k == GD_NONE ? 0 : (int32_t)(uint32_t)k;
    }
}

// ------------------------------------------------------------------------------------------------ host side
static inline int64_t gd_tiles(int X, int Y, int Z) {
    return (int64_t)((X + GD_TX - 1) / GD_TX) * ((Y + GD_TY - 1) / GD_TY) * ((Z + GD_TZ - 1) / GD_TZ);
}

static inline unsigned gd_stream_blocks(int64_t n) {
    const int64_t blocks = (n + 255) / 256;
    return (unsigned)(blocks > 16384 ? 16384 : blocks);
}

// the two activity maps, a byte per tile each
extern "C" size_t ru3d_geodesic_workspace_bytes(int X, int Y, int Z) {
    if (!bv_shape_ok(X, Y, Z)) return 0;
    return 2 * bv_align((size_t)gd_tiles(X, Y, Z));
}

extern "C" int ru3d_geodesic_init(const int32_t* seeds, uint64_t* keys, int X, int Y, int Z, int32_t* flags_dev, void* ws,
                                  size_t ws_bytes, void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    BV_REQUIRE_SHAPE("geodesic_init");
    RU3D_REQUIRE(seeds && keys && flags_dev && ws, "geodesic_init: bad argument (null pointer)");
    RU3D_REQUIRE((const void*)seeds != (const void*)keys, "geodesic_init: seeds and keys are one buffer");
    RU3D_REQUIRE(((uintptr_t)keys & 7) == 0, "geodesic_init: keys must be aligned to 8 bytes");
    const size_t need = ru3d_geodesic_workspace_bytes(X, Y, Z);
    RU3D_REQUIRE(ws_bytes >= need, "geodesic_init: workspace of %zu bytes, %zu needed", ws_bytes, need);
    hipStream_t st = as_stream(stream);
    if (hipMemsetAsync(flags_dev, 0, 2 * sizeof(int32_t), st) != hipSuccess ||
        hipMemsetAsync(ws, 0, need, st) != hipSuccess)
        return ru3d_check_launch("geodesic_init");
    const int64_t n = (int64_t)X * Y * Z;
    hipLaunchKernelGGL(gd_init_kernel, dim3(gd_stream_blocks(n)), dim3(256), 0, st, seeds, (gd_u64*)keys, n, flags_dev);
    return ru3d_check_launch("geodesic_init");
}

extern "C" int ru3d_geodesic_rounds(const uint64_t* allowed, int invert_allowed, uint64_t* keys, int X, int Y, int Z,
                                    const uint32_t* weights, uint32_t limit, int rounds, int first, int skip_idle,
                                    int32_t* changed_dev, int32_t* flags_dev, void* ws, size_t ws_bytes, void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    BV_REQUIRE_SHAPE("geodesic_rounds");
    RU3D_REQUIRE(keys && weights && changed_dev && flags_dev && ws, "geodesic_rounds: bad argument (null pointer)");
    RU3D_REQUIRE((const void*)allowed != (const void*)keys, "geodesic_rounds: allowed and keys are one buffer");
    RU3D_REQUIRE(((uintptr_t)keys & 7) == 0, "geodesic_rounds: keys must be aligned to 8 bytes");
    RU3D_REQUIRE(invert_allowed == 0 || invert_allowed == 1, "geodesic_rounds: invert_allowed %d (0 or 1)", invert_allowed);
    RU3D_REQUIRE(allowed || !invert_allowed, "geodesic_rounds: invert_allowed without an allowed mask");
    RU3D_REQUIRE(limit <= GD_UNLIMITED, "geodesic_rounds: limit %u (at most %u)", limit, GD_UNLIMITED);
    RU3D_REQUIRE(rounds >= 1 && rounds <= GD_MAX_ROUNDS, "geodesic_rounds: %d rounds (1 .. %d)", rounds, GD_MAX_ROUNDS);
    RU3D_REQUIRE(first == 0 || first == 1, "geodesic_rounds: first %d (0 or 1)", first);
    RU3D_REQUIRE(skip_idle == 0 || skip_idle == 1, "geodesic_rounds: skip_idle %d (0 or 1)", skip_idle);
    gd_weights wt;
    bool cube = false, any = false;
    for (int k = 0; k < 26; k++) {
        const int o = k < 13 ? k : k + 1;
        const int dx = o / 9 - 1, dy = (o / 3) % 3 - 1, dz = o % 3 - 1;
        RU3D_REQUIRE(weights[k] <= GD_MAX_WEIGHT, "geodesic_rounds: weight %u of step (%d, %d, %d) (0: no such step, else 1 .. %u)",
                     weights[k], dx, dy, dz, GD_MAX_WEIGHT);
        wt.w[k] = weights[k];
        any = any || weights[k] != 0;
        cube = cube || (weights[k] != 0 && dx * dx + dy * dy + dz * dz != 1);
    }
    RU3D_REQUIRE(any, "geodesic_rounds: every weight is 0 (no step at all)");
    const size_t need = ru3d_geodesic_workspace_bytes(X, Y, Z);
    RU3D_REQUIRE(ws_bytes >= need, "geodesic_rounds: workspace of %zu bytes, %zu needed", ws_bytes, need);
    const int XT = (X + GD_TX - 1) / GD_TX, YT = (Y + GD_TY - 1) / GD_TY, ZT = (Z + GD_TZ - 1) / GD_TZ;
    const int64_t tiles = (int64_t)XT * YT * ZT;
    hipStream_t st = as_stream(stream);
    if (hipMemsetAsync(changed_dev, 0, (size_t)rounds * sizeof(int32_t), st) != hipSuccess)
        return ru3d_check_launch("geodesic_rounds");
    // round r reads the map the round before it wrote; map 0 is what the last round of the call before left behind
    uint8_t* map[2] = {(uint8_t*)ws, (uint8_t*)ws + need / 2};
    const gd_u64 invert = invert_allowed ? ~0ull : 0ull;
    for (int r = 0; r < rounds; r++) {
        const int all_active = !skip_idle || (first && r == 0);
        if (cube)
            hipLaunchKernelGGL(gd_round_kernel<true>, dim3((unsigned)tiles), dim3(GD_THREADS), 0, st, (const gd_u64*)allowed,
                               invert, (gd_u64*)keys, X, Y, Z, XT, YT, ZT, wt, limit, all_active, map[r & 1], map[(r + 1) & 1],
                               changed_dev + r, flags_dev);
        else
            hipLaunchKernelGGL(gd_round_kernel<false>, dim3((unsigned)tiles), dim3(GD_THREADS), 0, st, (const gd_u64*)allowed,
                               invert, (gd_u64*)keys, X, Y, Z, XT, YT, ZT, wt, limit, all_active, map[r & 1], map[(r + 1) & 1],
                               changed_dev + r, flags_dev);
    }
    if ((rounds & 1) &&
        hipMemcpyAsync(map[0], map[1], (size_t)tiles, hipMemcpyDeviceToDevice, st) != hipSuccess)
        return ru3d_check_launch("geodesic_rounds");
    return ru3d_check_launch("geodesic_rounds");
}

extern "C" int ru3d_geodesic_split(const uint64_t* keys, uint32_t* dist, int32_t* labels, int X, int Y, int Z, void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    BV_REQUIRE_SHAPE("geodesic_split");
    RU3D_REQUIRE(keys && dist && labels, "geodesic_split: bad argument (null pointer)");
    RU3D_REQUIRE((const void*)dist != (const void*)labels && (const void*)keys != (const void*)dist &&
                     (const void*)keys != (const void*)labels,
                 "geodesic_split: not an in-place operation");
    const int64_t n = (int64_t)X * Y * Z;
    hipLaunchKernelGGL(gd_split_kernel, dim3(gd_stream_blocks(n)), dim3(256), 0, as_stream(stream), (const gd_u64*)keys, dist,
                       labels, n);
    return ru3d_check_launch("geodesic_split");
}
