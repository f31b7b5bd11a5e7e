// Morphometry of a label volume: what a report says about every kidney, tumour, cyst or connected component.
//
// `ids` is a uint8 class volume or an int32 component-label volume (components.hip), [X, Y, Z] with Z contiguous and
// X*Y*Z < 2^31.  Ids 1 .. count are measured; 0 and everything above `count` is skipped.  Every result is an integer
// count or a max / min of float64 values, made with integer atomics and 64-bit min / max, which do not depend on the
// order of arrival: two runs give identical bytes, and a numpy twin of the same definition gives the same numbers.
//   mo_moments_kernel       table[id][10] = n, Sx, Sy, Sz, Sxx, Syy, Szz, Sxy, Sxz, Syz over voxel indices (int64)
//   mo_faces_kernel         table[id][class of the neighbour | outside][axis] = faces of the id's voxels against it
//   mo_extents_kernel       min and max of three linear forms per id (the principal axes, given as `frames`)
//   mo_feret_count_kernel   candidates per id: the first and the last voxel of the id in every (x, y) row along Z
//   mo_feret_fill_kernel    their linear indices, grouped by id
//   mo_feret_rows_kernel    per candidate, the farthest candidate of its id under the metric G (LDS tiles, float64)
//   mo_feret_pick_kernel    per id, the largest of those with its pair
//
// One walk (mo_walk) feeds the first four: a thread owns 16 consecutive voxels per trip, aggregates what it meets in
// registers while the id does not change (a z-run of a row in closed form: n, Sz, Szz), and hands a finished run to the
// workgroup's LDS table.  The table is indexed by the cell itself when all cells fit (`direct`), and is an open-addressed
// hash otherwise; a cell that finds no slot goes straight to global memory.  The table leaves with one global atomic per
// used (slot, value).  So a giant component costs a workgroup one set of global atomics, and thousands of small ones
// spread over thousands of addresses.  All accumulation is 64-bit from the run onward.
#include "common.h"
#include "bitvol.h"

typedef unsigned long long mo_u64;
typedef long long mo_i64;

#define MO_SEG 16                           // voxels per thread and trip
#define MO_WIDE_SLOTS 256                   // LDS table of the 10-wide (moments) and 6-wide (extents) cells
#define MO_FLAT_SLOTS 2048                  // LDS table of the 1-wide cells (faces, candidate counts)
#define MO_PROBES 8
#define MO_TILE 256                         // candidates per LDS tile of the pair kernel
#define MO_ENC_PLUS_INF 0xfff0000000000000ull           // mo_encode(+inf), mo_encode(-inf)
#define MO_ENC_MINUS_INF 0x000fffffffffffffull

enum { MO_ADD = 0, MO_MINMAX = 1 };         // MINMAX: even values take the minimum, odd ones the maximum

// the order-preserving image of a double in the unsigned 64-bit integers
__device__ __forceinline__ mo_u64 mo_encode(double t) {
    const mo_i64 b = __double_as_longlong(t);
    return (mo_u64)(b ^ ((b >> 63) | (mo_i64)0x8000000000000000ull));
}
__device__ __forceinline__ double mo_decode(mo_u64 u) {
    const mo_i64 b = (u >> 63) ? (mo_i64)(u ^ 0x8000000000000000ull) : (mo_i64)~u;
    return __longlong_as_double(b);
}

// ------------------------------------------------------------------------------------------------ the LDS table
template <int OP>
__device__ __forceinline__ mo_u64 mo_identity(int w) {
    return OP == MO_ADD ? 0ull : ((w & 1) ? MO_ENC_MINUS_INF : MO_ENC_PLUS_INF);
}
template <int OP>
__device__ __forceinline__ void mo_join(mo_u64* p, mo_u64 v, int w) {
    if (OP == MO_ADD)
        atomicAdd(p, v);
    else if (w & 1)
        atomicMax(p, v);
    else
        atomicMin(p, v);
}

template <int W, int SLOTS, int OP>
__device__ __forceinline__ void mo_table_init(int* key, mo_u64* val) {
    for (int i = threadIdx.x; i < SLOTS; i += blockDim.x) key[i] = 0;
    for (int i = threadIdx.x; i < SLOTS * W; i += blockDim.x) val[i] = mo_identity<OP>(i % W);
    __syncthreads();
}

// v[0 .. W) joins cell `cell` (0 <= cell < cells)
template <int W, int SLOTS, int OP>
__device__ __forceinline__ void mo_table_put(bool direct, int cell, const mo_u64* v, int* key, mo_u64* val,
                                             mo_u64* __restrict__ global) {
    int slot = -1;
    if (direct) {
        slot = cell;
    } else {
        const unsigned h = ((unsigned)(cell + 1) * 2654435761u) >> 8;
        for (int p = 0; p < MO_PROBES; p++) {
            const int s = (int)((h + p) & (SLOTS - 1));
            const int old = atomicCAS(&key[s], 0, cell + 1);
            if (old == 0 || old == cell + 1) {
                slot = s;
                break;
            }
        }
    }
    if (slot >= 0) {
#pragma unroll
        for (int w = 0; w < W; w++)
            if (v[w] != mo_identity<OP>(w)) mo_join<OP>(val + slot * W + w, v[w], w);
    } else {
#pragma unroll
        for (int w = 0; w < W; w++)
            if (v[w] != mo_identity<OP>(w)) mo_join<OP>(global + (int64_t)cell * W + w, v[w], w);
    }
}

// every used (slot, value) of the workgroup's table joins global memory
template <int W, int SLOTS, int OP>
__device__ __forceinline__ void mo_table_flush(bool direct, int cells, const int* key, const mo_u64* val,
                                               mo_u64* __restrict__ global) {
    __syncthreads();
    for (int i = threadIdx.x; i < SLOTS * W; i += blockDim.x) {
        const int s = i / W, w = i % W;
        const int cell = direct ? (s < cells ? s : -1) : key[s] - 1;
        const mo_u64 v = val[i];
        if (cell >= 0 && v != mo_identity<OP>(w)) mo_join<OP>(global + (int64_t)cell * W + w, v, w);
    }
}

// ------------------------------------------------------------------------------------------------ the walk
template <typename ID>
__device__ __forceinline__ void mo_load_seg(const ID* __restrict__ ids, int64_t base, int64_t n, bool aligned, int* v) {
    if (aligned && base + MO_SEG <= n) {
        if (sizeof(ID) == 1) {
            const uint4 q = *reinterpret_cast<const uint4*>(ids + base);
            const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int b = 0; b < MO_SEG; b++) v[b] = (int)((w[b >> 2] >> (8 * (b & 3))) & 0xffu);
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int4 q = *reinterpret_cast<const int4*>(ids + base + 4 * k);
                v[4 * k] = q.x;
                v[4 * k + 1] = q.y;
                v[4 * k + 2] = q.z;
                v[4 * k + 3] = q.w;
            }
        }
    } else {
#pragma unroll
        for (int b = 0; b < MO_SEG; b++) v[b] = base + b < n ? (int)ids[base + b] : 0;
    }
}

// f.visit(id, x, y, z, linear index) for every voxel with 1 <= id <= count, 16 consecutive voxels per thread and trip
template <typename ID, typename F>
__device__ __forceinline__ void mo_walk(const ID* __restrict__ ids, int64_t n, int Y, int Z, int count, bool aligned, F& f) {
    const int64_t segs = (n + MO_SEG - 1) / MO_SEG;
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < segs; s += (int64_t)gridDim.x * blockDim.x) {
        const int64_t base = s * MO_SEG;
        int v[MO_SEG];
        mo_load_seg(ids, base, n, aligned, v);
        bool any = false;
#pragma unroll
        for (int b = 0; b < MO_SEG; b++) any |= (unsigned)(v[b] - 1) < (unsigned)count;
        if (!any) continue;
        const unsigned row = (unsigned)base / (unsigned)Z;          // base < 2^31
        int z = (int)(base - (int64_t)row * Z), y = (int)(row % (unsigned)Y), x = (int)(row / (unsigned)Y);
#pragma unroll
        for (int b = 0; b < MO_SEG; b++) {
            if ((unsigned)(v[b] - 1) < (unsigned)count) f.visit(v[b], x, y, z, base + b);
            if (++z == Z) {
                z = 0;
                if (++y == Y) {
                    y = 0;
                    x++;
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ moments
struct mo_moment_run {
    bool direct;
    int* key;
    mo_u64* val;
    mo_u64* global;
    int id, x, y;
    mo_i64 n, sz, szz;                      // the open z-run of row (x, y)
    mo_i64 a[10];                           // the finished runs of `id`
    __device__ __forceinline__ void fold() {
        if (n) {
            const mo_i64 X = x, Yv = y;
            a[0] += n;
            a[1] += X * n;
            a[2] += Yv * n;
            a[3] += sz;
            a[4] += X * X * n;
            a[5] += Yv * Yv * n;
            a[6] += szz;
            a[7] += X * Yv * n;
            a[8] += X * sz;
            a[9] += Yv * sz;
        }
        n = sz = szz = 0;
    }
    __device__ __forceinline__ void flush() {
        fold();
        if (id > 0 && a[0]) {
            mo_u64 v[10];
#pragma unroll
            for (int w = 0; w < 10; w++) {
                v[w] = (mo_u64)a[w];
                a[w] = 0;
            }
            mo_table_put<10, MO_WIDE_SLOTS, MO_ADD>(direct, id - 1, v, key, val, global);
        }
    }
    __device__ __forceinline__ void visit(int k, int vx, int vy, int vz, int64_t) {
        if (k != id) {
            flush();
            id = k;
            x = vx;
            y = vy;
        } else if (vx != x || vy != y) {
            fold();
            x = vx;
            y = vy;
        }
        n++;
        sz += vz;
        szz += (mo_i64)vz * vz;
    }
};

template <typename ID>
__global__ __launch_bounds__(256) void mo_moments_kernel(const ID* __restrict__ ids, int64_t n, int Y, int Z, int count,
                                                         int aligned, int direct, mo_u64* __restrict__ table) {
    __shared__ int key[MO_WIDE_SLOTS];
    __shared__ mo_u64 val[MO_WIDE_SLOTS * 10];
    mo_table_init<10, MO_WIDE_SLOTS, MO_ADD>(key, val);
    mo_moment_run run;
    run.direct = direct != 0;
    run.key = key;
    run.val = val;
    run.global = table;
    run.id = 0;
    run.x = run.y = 0;
    run.n = run.sz = run.szz = 0;
#pragma unroll
    for (int w = 0; w < 10; w++) run.a[w] = 0;
    mo_walk(ids, n, Y, Z, count, aligned != 0, run);
    run.flush();
    mo_table_flush<10, MO_WIDE_SLOTS, MO_ADD>(direct != 0, count, key, val, table);
}

// ------------------------------------------------------------------------------------------------ flat cells
// a run of equal cells of one thread (faces, candidate counts)
struct mo_cell_run {
    bool direct;
    int* key;
    mo_u64* val;
    mo_u64* global;
    int cell;
    mo_i64 n;
    __device__ __forceinline__ void flush() {
        if (n) {
            const mo_u64 v = (mo_u64)n;
            mo_table_put<1, MO_FLAT_SLOTS, MO_ADD>(direct, cell, &v, key, val, global);
        }
        n = 0;
    }
    __device__ __forceinline__ void add(int c) {
        if (c != cell) {
            flush();
            cell = c;
        }
        n++;
    }
};

template <typename ID>
struct mo_face_visitor {
    mo_cell_run run;
    const ID* ids;
    const uint8_t* other;
    int X, Y, Z, M;                         // M = num_other: column M is "outside the volume"
    __device__ __forceinline__ void side(int k, int64_t q, bool inside, int axis) {
        if (!inside) {
            run.add(((k - 1) * (M + 1) + M) * 3 + axis);
        } else if ((int)ids[q] != k) {
            const int c = other[q];
            if (c < M) run.add(((k - 1) * (M + 1) + c) * 3 + axis);
        }
    }
    __device__ __forceinline__ void visit(int k, int x, int y, int z, int64_t p) {
        const int64_t sx = (int64_t)Y * Z;
        side(k, p - sx, x > 0, 0);
        side(k, p + sx, x < X - 1, 0);
        side(k, p - Z, y > 0, 1);
        side(k, p + Z, y < Y - 1, 1);
        side(k, p - 1, z > 0, 2);
        side(k, p + 1, z < Z - 1, 2);
    }
};

template <typename ID>
__global__ __launch_bounds__(256) void mo_faces_kernel(const ID* __restrict__ ids, const uint8_t* __restrict__ other,
                                                       int X, int Y, int Z, int count, int M, int aligned, int direct,
                                                       mo_u64* __restrict__ table) {
    __shared__ int key[MO_FLAT_SLOTS];
    __shared__ mo_u64 val[MO_FLAT_SLOTS];
    mo_table_init<1, MO_FLAT_SLOTS, MO_ADD>(key, val);
    mo_face_visitor<ID> f;
    f.run.direct = direct != 0;
    f.run.key = key;
    f.run.val = val;
    f.run.global = table;
    f.run.cell = -1;
    f.run.n = 0;
    f.ids = ids;
    f.other = other;
    f.X = X;
    f.Y = Y;
    f.Z = Z;
    f.M = M;
    mo_walk(ids, (int64_t)X * Y * Z, Y, Z, count, aligned != 0, f);
    f.run.flush();
    mo_table_flush<1, MO_FLAT_SLOTS, MO_ADD>(direct != 0, count * (M + 1) * 3, key, val, table);
}

// ------------------------------------------------------------------------------------------------ extents
struct mo_extent_run {
    bool direct;
    int* key;
    mo_u64* val;
    mo_u64* global;
    const double* frames;
    int id, x, y, z0, z1;                   // the open z-run of row (x, y): z0 .. z1, none when z1 < z0
    double f[12];                           // the id's three rows (ax, ay, az, b)
    double lo[3], hi[3];
    // a linear form takes its extremes over a z-run at the run's two ends
    __device__ __forceinline__ void fold() {
        if (z1 >= z0) {
#pragma unroll
            for (int a = 0; a < 3; a++) {
                const double t0 = f[4 * a] * x + f[4 * a + 1] * y + f[4 * a + 2] * z0 + f[4 * a + 3];
                const double t1 = f[4 * a] * x + f[4 * a + 1] * y + f[4 * a + 2] * z1 + f[4 * a + 3];
                lo[a] = fmin(lo[a], fmin(t0, t1));
                hi[a] = fmax(hi[a], fmax(t0, t1));
            }
        }
        z1 = -1;
        z0 = 0;
    }
    __device__ __forceinline__ void flush() {
        fold();
        if (id > 0) {
            mo_u64 v[6];
#pragma unroll
            for (int a = 0; a < 3; a++) {
                v[2 * a] = mo_encode(lo[a]);
                v[2 * a + 1] = mo_encode(hi[a]);
            }
            mo_table_put<6, MO_WIDE_SLOTS, MO_MINMAX>(direct, id - 1, v, key, val, global);
        }
    }
    __device__ __forceinline__ void visit(int k, int vx, int vy, int vz, int64_t) {
        if (k != id) {
            flush();
            id = k;
#pragma unroll
            for (int i = 0; i < 12; i++) f[i] = frames[(int64_t)(k - 1) * 12 + i];
#pragma unroll
            for (int a = 0; a < 3; a++) {
                lo[a] = __longlong_as_double(0x7ff0000000000000ll);
                hi[a] = __longlong_as_double((mo_i64)0xfff0000000000000ull);
            }
            x = vx;
            y = vy;
            z0 = vz;
        } else if (vx != x || vy != y) {
            fold();
            x = vx;
            y = vy;
            z0 = vz;
        } else if (z1 < z0) {
            z0 = vz;
        }
        z1 = vz;
    }
};

template <typename ID>
__global__ __launch_bounds__(256) void mo_extents_kernel(const ID* __restrict__ ids, int64_t n, int Y, int Z, int count,
                                                         int aligned, int direct, const double* __restrict__ frames,
                                                         mo_u64* __restrict__ out) {
    __shared__ int key[MO_WIDE_SLOTS];
    __shared__ mo_u64 val[MO_WIDE_SLOTS * 6];
    mo_table_init<6, MO_WIDE_SLOTS, MO_MINMAX>(key, val);
    mo_extent_run run;
    run.direct = direct != 0;
    run.key = key;
    run.val = val;
    run.global = out;
    run.frames = frames;
    run.id = 0;
    run.x = run.y = run.z0 = 0;
    run.z1 = -1;
    mo_walk(ids, n, Y, Z, count, aligned != 0, run);
    run.flush();
    mo_table_flush<6, MO_WIDE_SLOTS, MO_MINMAX>(direct != 0, count, key, val, out);
}

// p[i] = even / odd by the parity of i
__global__ __launch_bounds__(256) void mo_fill_kernel(mo_u64* __restrict__ p, int64_t n, mo_u64 even, mo_u64 odd) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) p[i] = (i & 1) ? odd : even;
}
__global__ __launch_bounds__(256) void mo_decode_kernel(mo_u64* __restrict__ p, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        reinterpret_cast<double*>(p)[i] = mo_decode(p[i]);
}

// ------------------------------------------------------------------------------------------------ Feret candidates
// the voxel at z of a row is the first or the last of its id in that row (a voxel strictly between two others of its id
// on a line is no extreme point of the id's voxel set, so it ends no diameter)
template <typename ID>
__device__ __forceinline__ bool mo_is_candidate(const ID* __restrict__ row, int Z, int z, int k) {
    bool first = true;
    for (int t = z - 1; t >= 0; t--)
        if ((int)row[t] == k) {
            first = false;
            break;
        }
    if (first) return true;
    for (int t = z + 1; t < Z; t++)
        if ((int)row[t] == k) return false;
    return true;
}

template <typename ID>
struct mo_candidate_counter {
    mo_cell_run run;
    const ID* ids;
    int Z;
    __device__ __forceinline__ void visit(int k, int, int, int z, int64_t p) {
        if (mo_is_candidate(ids + (p - z), Z, z, k)) run.add(k - 1);
    }
};

template <typename ID>
__global__ __launch_bounds__(256) void mo_feret_count_kernel(const ID* __restrict__ ids, int64_t n, int Y, int Z, int count,
                                                             int aligned, int direct, mo_u64* __restrict__ counts) {
    __shared__ int key[MO_FLAT_SLOTS];
    __shared__ mo_u64 val[MO_FLAT_SLOTS];
    mo_table_init<1, MO_FLAT_SLOTS, MO_ADD>(key, val);
    mo_candidate_counter<ID> f;
    f.run.direct = direct != 0;
    f.run.key = key;
    f.run.val = val;
    f.run.global = counts;
    f.run.cell = -1;
    f.run.n = 0;
    f.ids = ids;
    f.Z = Z;
    mo_walk(ids, n, Y, Z, count, aligned != 0, f);
    f.run.flush();
    mo_table_flush<1, MO_FLAT_SLOTS, MO_ADD>(direct != 0, count, key, val, counts);
}

// One thread per voxel.  The lanes of a wave that hold candidates of one id claim their places with one atomic.
template <typename ID>
__global__ __launch_bounds__(256) void mo_feret_fill_kernel(const ID* __restrict__ ids, int64_t n, int Z, int count,
                                                            const mo_i64* __restrict__ starts, mo_u64* __restrict__ cursor,
                                                            int* __restrict__ cand, int64_t capacity) {
    const int lane = threadIdx.x & 63;
    const int64_t whole = (n + 63) & ~(int64_t)63;              // a wave stays together through the loop
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < whole; i += (int64_t)gridDim.x * 256) {
        int k = 0;
        bool pending = false;
        if (i < n) {
            k = (int)ids[i];
            if ((unsigned)(k - 1) < (unsigned)count) {
                const int z = (int)(i % Z);
                pending = mo_is_candidate(ids + (i - z), Z, z, k);
            }
        }
        mo_u64 todo = __ballot(pending);
        while (todo) {
            const int leader = __ffsll((mo_i64)todo) - 1;
            const int k0 = __shfl(k, leader, 64);
            const bool mine = pending && k == k0;
            const mo_u64 group = __ballot(mine);
            mo_u64 at = 0;
            if (lane == leader) at = atomicAdd(&cursor[k0 - 1], (mo_u64)__popcll(group));
            const unsigned at_lo = __shfl((unsigned)at, leader, 64), at_hi = __shfl((unsigned)(at >> 32), leader, 64);
            if (mine) {
                const mo_i64 pos = starts[k0 - 1] + (mo_i64)((mo_u64)at_hi << 32 | at_lo) +
                                   __popcll(group & (((mo_u64)1 << lane) - 1));
                if (pos >= 0 && pos < capacity) cand[pos] = (int)i;
                pending = false;
            }
            todo &= ~group;
        }
    }
}

// ------------------------------------------------------------------------------------------------ Feret pairs
struct mo_metric {
    double g00, g11, g22, g01, g02, g12;    // the off-diagonal ones doubled
};
__device__ __forceinline__ double mo_dist2(const mo_metric& g, int dx, int dy, int dz) {
    const double x = dx, y = dy, z = dz;
    return x * (g.g00 * x + g.g01 * y + g.g02 * z) + y * (g.g11 * y + g.g12 * z) + z * (g.g22 * z);
}

// One thread per entry of the candidate buffer.  The groups of the entries of a workgroup form one stretch of the
// buffer; it passes through LDS in tiles, and every thread looks at the part of a tile that belongs to its own group.
// row_d2[e] = the largest squared distance from candidate e to a candidate of its id, row_partner[e] = the linear index
// of the one that reaches it (the smallest on a tie); -1 / -1 for an entry that is no voxel of a measured id.
template <typename ID>
__global__ __launch_bounds__(MO_TILE) void mo_feret_rows_kernel(const ID* __restrict__ ids, int64_t n, int Y, int Z, int count,
                                                                const int* __restrict__ cand, int total,
                                                                const mo_i64* __restrict__ starts,
                                                                const mo_i64* __restrict__ counts, mo_metric g,
                                                                double* __restrict__ row_d2, int* __restrict__ row_partner) {
    __shared__ int tx[MO_TILE], ty[MO_TILE], tz[MO_TILE], tl[MO_TILE];
    __shared__ int s_lo, s_hi;
    if (threadIdx.x == 0) {
        s_lo = total;
        s_hi = 0;
    }
    __syncthreads();
    const int e = blockIdx.x * MO_TILE + threadIdx.x;
    int lo = 0, hi = 0, x = 0, y = 0, z = 0;
    bool valid = false;
    if (e < total) {
        const int lin = cand[e];
        if ((unsigned)lin < (unsigned)n) {
            const int k = (int)ids[lin];
            if ((unsigned)(k - 1) < (unsigned)count) {
                const mo_i64 s = starts[k - 1], c = counts[k - 1];
                lo = (int)(s < 0 ? 0 : (s > total ? total : s));
                hi = (int)(c < 0 || s + c < lo ? lo : (s + c > total ? total : s + c));
                valid = hi > lo;
                z = lin % Z;
                y = (lin / Z) % Y;
                x = lin / Z / Y;
            }
        }
    }
    if (valid) {
        atomicMin(&s_lo, lo);
        atomicMax(&s_hi, hi);
    }
    __syncthreads();
    const int blo = s_lo, bhi = s_hi;
    double best = -1.0;
    int partner = -1;
    for (int t = blo; t < bhi; t += MO_TILE) {
        const int j = t + threadIdx.x;
        int lin = -1;
        if (j < bhi) lin = cand[j];
        if ((unsigned)lin >= (unsigned)n) lin = -1;
        tl[threadIdx.x] = lin;
        tz[threadIdx.x] = lin < 0 ? 0 : lin % Z;
        ty[threadIdx.x] = lin < 0 ? 0 : (lin / Z) % Y;
        tx[threadIdx.x] = lin < 0 ? 0 : lin / Z / Y;
        __syncthreads();
        if (valid) {
            const int j0 = (lo > t ? lo : t) - t, j1 = (hi < t + MO_TILE ? hi : t + MO_TILE) - t;
            for (int jj = j0; jj < j1; jj++) {
                const int lj = tl[jj];
                if (lj < 0) continue;
                const double d = mo_dist2(g, x - tx[jj], y - ty[jj], z - tz[jj]);
                if (d > best || (d == best && lj < partner)) {
                    best = d;
                    partner = lj;
                }
            }
        }
        __syncthreads();
    }
    if (e < total) {
        row_d2[e] = best;
        row_partner[e] = partner;
    }
}

// One wave per id: the largest row maximum; on a tie the smallest candidate, then its smallest partner.
__global__ __launch_bounds__(256) void mo_feret_pick_kernel(const int* __restrict__ cand, int total,
                                                            const mo_i64* __restrict__ starts,
                                                            const mo_i64* __restrict__ counts, int count, int Y, int Z,
                                                            const double* __restrict__ row_d2,
                                                            const int* __restrict__ row_partner, double* __restrict__ out_d2,
                                                            int* __restrict__ out_pair) {
    const int lane = threadIdx.x & 63;
    for (int k = blockIdx.x * 4 + (threadIdx.x >> 6); k < count; k += gridDim.x * 4) {
        const mo_i64 s = starts[k], c = counts[k];
        const int lo = (int)(s < 0 ? 0 : (s > total ? total : s));
        const int hi = (int)(c < 0 || s + c < lo ? lo : (s + c > total ? total : s + c));
        double best = -1.0;
        int a = -1, b = -1;
        for (int e = lo + lane; e < hi; e += 64) {
            const double d = row_d2[e];
            const int ea = cand[e], eb = row_partner[e];
            if (eb >= 0 && (d > best || (d == best && (ea < a || (ea == a && eb < b))))) {
                best = d;
                a = ea;
                b = eb;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const mo_i64 bits = __double_as_longlong(best);
            const unsigned d_lo = __shfl_xor((unsigned)bits, o, 64), d_hi = __shfl_xor((unsigned)((mo_u64)bits >> 32), o, 64);
            const double d = __longlong_as_double((mo_i64)((mo_u64)d_hi << 32 | d_lo));
            const int oa = __shfl_xor(a, o, 64), ob = __shfl_xor(b, o, 64);
            if (ob >= 0 && (b < 0 || d > best || (d == best && (oa < a || (oa == a && ob < b))))) {
                best = d;
                a = oa;
                b = ob;
            }
        }
        if (lane == 0) {
            out_d2[k] = best;
            int* p = out_pair + (int64_t)k * 6;
            p[0] = a < 0 ? -1 : a / Z / Y;
            p[1] = a < 0 ? -1 : (a / Z) % Y;
            p[2] = a < 0 ? -1 : a % Z;
            p[3] = b < 0 ? -1 : b / Z / Y;
            p[4] = b < 0 ? -1 : (b / Z) % Y;
            p[5] = b < 0 ? -1 : b % Z;
        }
    }
}

// ------------------------------------------------------------------------------------------------ host side
static inline int mo_blocks(int64_t work_items) {
    int64_t b = (work_items + 255) / 256;
    const int64_t cap = (int64_t)ru3d_get_cu_budget() * 8;
    b = b > cap ? cap : b;
    return (int)(b < 1 ? 1 : b);
}
static inline int mo_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }
// the sums of squares of the moments stay below 2^63
static inline bool mo_moments_fit(int X, int Y, int Z) {
    int m = X > Y ? X : Y;
    m = (m > Z ? m : Z) - 1;
    const unsigned __int128 worst = (unsigned __int128)((int64_t)X * Y * Z) * (unsigned __int128)((int64_t)m * m);
    return worst < ((unsigned __int128)1 << 63);
}

#define MO_REQUIRE_IDS(what)                                                                                          \
    BV_REQUIRE_SHAPE(what);                                                                                           \
    RU3D_REQUIRE(id_bytes == 1 || id_bytes == 4, what ": ids of %d bytes (1 = uint8 classes, 4 = int32 components)",   \
                 id_bytes);                                                                                           \
    RU3D_REQUIRE(count >= 0, what ": count %d", count)

#define MO_LAUNCH(kernel, grid, block, ...)                                                                            \
    do {                                                                                                               \
        if (id_bytes == 1)                                                                                             \
            hipLaunchKernelGGL(kernel<uint8_t>, grid, block, 0, st, (const uint8_t*)ids, __VA_ARGS__);                 \
        else                                                                                                           \
            hipLaunchKernelGGL(kernel<int32_t>, grid, block, 0, st, (const int32_t*)ids, __VA_ARGS__);                 \
    } while (0)

extern "C" int ru3d_label_moments(const void* ids, int id_bytes, int X, int Y, int Z, int count, int64_t* table,
                                  void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    MO_REQUIRE_IDS("label_moments");
    RU3D_REQUIRE(mo_moments_fit(X, Y, Z), "label_moments: the second moments of a %dx%dx%d volume can pass 2^63", X, Y, Z);
    if (count == 0) return 0;
    RU3D_REQUIRE(ids && table, "label_moments: bad argument (null pointer)");
    hipStream_t st = as_stream(stream);
    const int64_t n = (int64_t)X * Y * Z, cells = (int64_t)count * 10;
    hipLaunchKernelGGL(mo_fill_kernel, dim3(mo_blocks(cells)), dim3(256), 0, st, (mo_u64*)table, cells, 0ull, 0ull);
    MO_LAUNCH(mo_moments_kernel, dim3(mo_blocks((n + MO_SEG - 1) / MO_SEG)), dim3(256), n, Y, Z, count, mo_aligned(ids),
              (int)(count <= MO_WIDE_SLOTS), (mo_u64*)table);
    return ru3d_check_launch("label_moments");
}

extern "C" int ru3d_label_faces(const void* ids, int id_bytes, const uint8_t* other, int num_other, int X, int Y, int Z,
                                int count, int64_t* table, void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    MO_REQUIRE_IDS("label_faces");
    RU3D_REQUIRE(num_other >= 0 && num_other <= 256, "label_faces: %d classes of the other volume (0 .. 256)", num_other);
    const int64_t cells = (int64_t)count * (num_other + 1) * 3;
    RU3D_REQUIRE(cells < ((int64_t)1 << 31), "label_faces: a table of %lld cells (below 2^31)", (long long)cells);
    if (count == 0) return 0;
    RU3D_REQUIRE(ids && other && table, "label_faces: bad argument (null pointer)");
    hipStream_t st = as_stream(stream);
    const int64_t n = (int64_t)X * Y * Z;
    hipLaunchKernelGGL(mo_fill_kernel, dim3(mo_blocks(cells)), dim3(256), 0, st, (mo_u64*)table, cells, 0ull, 0ull);
    MO_LAUNCH(mo_faces_kernel, dim3(mo_blocks((n + MO_SEG - 1) / MO_SEG)), dim3(256), other, X, Y, Z, count, num_other,
              mo_aligned(ids), (int)(cells <= MO_FLAT_SLOTS), (mo_u64*)table);
    return ru3d_check_launch("label_faces");
}

extern "C" int ru3d_label_extents(const void* ids, int id_bytes, int X, int Y, int Z, int count, const double* frames,
                                  double* out, void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    MO_REQUIRE_IDS("label_extents");
    if (count == 0) return 0;
    RU3D_REQUIRE(ids && frames && out, "label_extents: bad argument (null pointer)");
    hipStream_t st = as_stream(stream);
    const int64_t n = (int64_t)X * Y * Z, cells = (int64_t)count * 6;
    hipLaunchKernelGGL(mo_fill_kernel, dim3(mo_blocks(cells)), dim3(256), 0, st, (mo_u64*)out, cells, MO_ENC_PLUS_INF,
                       MO_ENC_MINUS_INF);
    MO_LAUNCH(mo_extents_kernel, dim3(mo_blocks((n + MO_SEG - 1) / MO_SEG)), dim3(256), n, Y, Z, count, mo_aligned(ids),
              (int)(count <= MO_WIDE_SLOTS), frames, (mo_u64*)out);
    hipLaunchKernelGGL(mo_decode_kernel, dim3(mo_blocks(cells)), dim3(256), 0, st, (mo_u64*)out, cells);
    return ru3d_check_launch("label_extents");
}

extern "C" int ru3d_label_feret_count(const void* ids, int id_bytes, int X, int Y, int Z, int count, int64_t* counts,
                                      void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    MO_REQUIRE_IDS("label_feret_count");
    if (count == 0) return 0;
    RU3D_REQUIRE(ids && counts, "label_feret_count: bad argument (null pointer)");
    hipStream_t st = as_stream(stream);
    const int64_t n = (int64_t)X * Y * Z;
    hipLaunchKernelGGL(mo_fill_kernel, dim3(mo_blocks(count)), dim3(256), 0, st, (mo_u64*)counts, (int64_t)count, 0ull, 0ull);
    MO_LAUNCH(mo_feret_count_kernel, dim3(mo_blocks((n + MO_SEG - 1) / MO_SEG)), dim3(256), n, Y, Z, count, mo_aligned(ids),
              (int)(count <= MO_FLAT_SLOTS), (mo_u64*)counts);
    return ru3d_check_launch("label_feret_count");
}

extern "C" int ru3d_label_feret_fill(const void* ids, int id_bytes, int X, int Y, int Z, int count, const int64_t* starts,
                                     int64_t* filled, int32_t* candidates, int64_t capacity, void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    MO_REQUIRE_IDS("label_feret_fill");
    RU3D_REQUIRE(capacity >= 0 && capacity < ((int64_t)1 << 31), "label_feret_fill: capacity %lld (0 .. 2^31 - 1)",
                 (long long)capacity);
    if (count == 0) return 0;
    RU3D_REQUIRE(ids && starts && filled && (candidates || capacity == 0), "label_feret_fill: bad argument (null pointer)");
    hipStream_t st = as_stream(stream);
    const int64_t n = (int64_t)X * Y * Z;
    hipLaunchKernelGGL(mo_fill_kernel, dim3(mo_blocks(count)), dim3(256), 0, st, (mo_u64*)filled, (int64_t)count, 0ull, 0ull);
    MO_LAUNCH(mo_feret_fill_kernel, dim3(mo_blocks(n)), dim3(256), n, Z, count, (const mo_i64*)starts, (mo_u64*)filled,
              (int*)candidates, capacity);
    return ru3d_check_launch("label_feret_fill");
}

extern "C" int ru3d_label_feret(const void* ids, int id_bytes, int X, int Y, int Z, int count, const int32_t* candidates,
                                int64_t total, const int64_t* starts, const int64_t* counts, const double* gram,
                                double* row_d2, int32_t* row_partner, double* out_d2, int32_t* out_pair, void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    MO_REQUIRE_IDS("label_feret");
    RU3D_REQUIRE(total >= 0 && total < ((int64_t)1 << 31), "label_feret: %lld candidates (0 .. 2^31 - 1)", (long long)total);
    if (count == 0) return 0;
    RU3D_REQUIRE(ids && starts && counts && gram && out_d2 && out_pair && (total == 0 || (candidates && row_d2 && row_partner)),
                 "label_feret: bad argument (null pointer)");
    for (int i = 0; i < 6; i++) RU3D_REQUIRE(gram[i] == gram[i], "label_feret: the metric holds a NaN (entry %d)", i);
    hipStream_t st = as_stream(stream);
    const int64_t n = (int64_t)X * Y * Z;
    mo_metric g;                              // gram = (G00, G11, G22, G01, G02, G12) on the host
    g.g00 = gram[0];
    g.g11 = gram[1];
    g.g22 = gram[2];
    g.g01 = 2.0 * gram[3];
    g.g02 = 2.0 * gram[4];
    g.g12 = 2.0 * gram[5];
    if (total > 0)
        MO_LAUNCH(mo_feret_rows_kernel, dim3((unsigned)((total + MO_TILE - 1) / MO_TILE)), dim3(MO_TILE), n, Y, Z, count,
                  (const int*)candidates, (int)total, (const mo_i64*)starts, (const mo_i64*)counts, g, row_d2,
                  (int*)row_partner);
    hipLaunchKernelGGL(mo_feret_pick_kernel, dim3(mo_blocks((int64_t)count * 64)), dim3(256), 0, st, (const int*)candidates,
                       (int)total, (const mo_i64*)starts, (const mo_i64*)counts, count, Y, Z, (const double*)row_d2,
                       (const int*)row_partner, out_d2, (int*)out_pair);
    return ru3d_check_launch("label_feret");
}
