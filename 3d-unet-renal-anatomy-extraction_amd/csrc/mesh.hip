// Triangle mesh of a bit-packed mask: the faces between a set voxel and an unset one (the "cuberille"), the lattice
// edge graph of its vertices, umbrella smoothing on that graph and the area / enclosed volume of a triangle list.
// Packed masks, the bounded word fetch, the z-neighbour view and the count / scan / rank pieces are those of bitvol.h.
// The contract (vertex, quad and triangle order, the smoothing expression, the sums) is written down in include/ru3d.h;
// everything up to the smoothing is integers, and the float64 kernels are compiled with contraction off, so a numpy
// restatement of the contract can be compared with ==.
//
// The hot path is words and popcounts, not a voxel loop:
//   mh_flag_kernel     corner flags as packed words of Z + 1 bits per corner row (i, j): from the four voxel rows
//                      around it, with s = the row shifted up one bit (carry from the word below),
//                      flag = OR(r | s) & ~AND(r & s).  One word per lane, popcounts summed per 256-word chunk.
//   mh_quad_count_kernel   E_d = w & ~neighbour_d per mask word (four row neighbours, two in-row shifts with carry),
//                      popcounts summed per chunk.
//   mh_scan_kernel     bitvol.h's scan of the chunk counts, one workgroup per list (vertices, quads), 64-bit totals.
//   mh_prefix_kernel   the number of vertices in front of every flag word (int32): a corner's vertex number is
//                      prefix[word] + popcount(flag & below(k)); no dense volume of corner numbers exists anywhere.
//   mh_vertex_kernel   per flag word: corners and the six neighbours of its vertices.  A lattice edge belongs to the
//                      graph iff its four voxels are mixed, which is the same OR / AND over two of the four rows (x and
//                      y edges) or over the raw / shifted words of all four (z edges); the z neighbours are rank -+ 1.
//   mh_quad_kernel     per mask word: ranks by an in-chunk scan, the eight corner numbers of a surface voxel from the
//                      flag words and prefixes of its four corner rows, two triangles per exposed face.
//   mh_smooth_kernel   one umbrella step, one vertex per lane, not in place.
//   mh_measure_partial / mh_measure_final   sums of |cross| and of the triple products over a fixed partition (2048
//                      faces per partial whatever the grid) and fixed trees, as ed_reduce in distance.hip.
// Every store is guarded by the caller's capacity, every index read from a caller's table is range-checked.
#include <math.h>
#include "common.h"
#include "bitvol.h"

#pragma clang fp contract(off)

typedef unsigned long long mh_u64;

#define MH_CHUNK 256                      // words of a chunk = threads of its workgroup
#define MH_RTHREADS 256
#define MH_RCHUNK 2048                    // faces per partial of the measures

struct mh_dims {
    int X, Y, Z, W, CW;                   // W words per voxel row, CW = Z / 64 + 1 words per corner row
    int64_t mwords, fwords;               // X Y W mask words, (X + 1)(Y + 1) CW flag words
    mh_u64 tail;                          // the bits at z >= Z of a row's last word
};

// word w of voxel row (x, y) without the caller's tail bits; 0 outside the volume
__device__ __forceinline__ mh_u64 mh_word(const mh_u64* __restrict__ bits, const mh_dims& g, int x, int y, int w) {
    return bv_word_masked(bits, g.X, g.Y, g.W, g.tail, x, y, w);
}

// the four voxel rows around corner row (i, j), word cw: n = 0 .. 3 is (i-1, j-1), (i-1, j), (i, j-1), (i, j).
// r = the voxels z = k of bit k, s = the voxels z = k - 1 (the row shifted up one bit, carry from word cw - 1)
struct mh_rows {
    mh_u64 r[4], s[4];
};
__device__ __forceinline__ mh_rows mh_load_rows(const mh_u64* __restrict__ bits, const mh_dims& g, int i, int j, int cw) {
    mh_rows v;
#pragma unroll
    for (int n = 0; n < 4; n++) {
        const int x = i - 1 + (n >> 1), y = j - 1 + (n & 1);
        const mh_u64 cur = mh_word(bits, g, x, y, cw), prev = mh_word(bits, g, x, y, cw - 1);
        v.r[n] = cur;
        v.s[n] = bv_zdown(prev, cur);
    }
    return v;
}
// neither all set nor all unset, over the rows a and b (both voxels of z per row)
__device__ __forceinline__ mh_u64 mh_mixed2(const mh_rows& v, int a, int b) {
    return ((v.r[a] | v.s[a]) | (v.r[b] | v.s[b])) & ~((v.r[a] & v.s[a]) & (v.r[b] & v.s[b]));
}
__device__ __forceinline__ mh_u64 mh_mixed4(const mh_u64* q) {
    return (q[0] | q[1] | q[2] | q[3]) & ~(q[0] & q[1] & q[2] & q[3]);
}
__device__ __forceinline__ mh_u64 mh_flag(const mh_rows& v) {
    return ((v.r[0] | v.s[0]) | (v.r[1] | v.s[1]) | (v.r[2] | v.s[2]) | (v.r[3] | v.s[3])) &
           ~((v.r[0] & v.s[0]) & (v.r[1] & v.s[1]) & (v.r[2] & v.s[2]) & (v.r[3] & v.s[3]));
}
__device__ __forceinline__ mh_u64 mh_below(int b) { return (1ull << b) - 1ull; }      // b in 0 .. 63

// exposed faces of mask word (x, y, w) in the contract's direction order -x, +x, -y, +y, -z, +z
struct mh_faces {
    mh_u64 e[6];
};
__device__ __forceinline__ mh_faces mh_exposed(const mh_u64* __restrict__ bits, const mh_dims& g, int x, int y, int w) {
    mh_faces f;
    const mh_u64 m = mh_word(bits, g, x, y, w);
    if (!m) {
#pragma unroll
        for (int d = 0; d < 6; d++) f.e[d] = 0ull;
        return f;
    }
    f.e[0] = m & ~mh_word(bits, g, x - 1, y, w);
    f.e[1] = m & ~mh_word(bits, g, x + 1, y, w);
    f.e[2] = m & ~mh_word(bits, g, x, y - 1, w);
    f.e[3] = m & ~mh_word(bits, g, x, y + 1, w);
    f.e[4] = m & ~bv_zdown(mh_word(bits, g, x, y, w - 1), m);
    f.e[5] = m & ~bv_zup(m, mh_word(bits, g, x, y, w + 1));
    return f;
}

__global__ __launch_bounds__(MH_CHUNK) void mh_flag_kernel(const mh_u64* __restrict__ bits, mh_dims g,
                                                           mh_u64* __restrict__ flags, int* __restrict__ counts) {
    const int64_t i = (int64_t)blockIdx.x * MH_CHUNK + threadIdx.x;
    mh_u64 f = 0ull;
    if (i < g.fwords) {
        const int64_t row = i / g.CW;
        f = mh_flag(mh_load_rows(bits, g, (int)(row / (g.Y + 1)), (int)(row % (g.Y + 1)), (int)(i - row * g.CW)));
        flags[i] = f;
    }
    bv_chunk_sum(__popcll(f), counts);
}

__global__ __launch_bounds__(MH_CHUNK) void mh_quad_count_kernel(const mh_u64* __restrict__ bits, mh_dims g,
                                                                 int* __restrict__ counts) {
    const int64_t i = (int64_t)blockIdx.x * MH_CHUNK + threadIdx.x;
    int c = 0;
    if (i < g.mwords) {
        const int64_t row = i / g.W;
        const mh_faces f = mh_exposed(bits, g, (int)(row / g.Y), (int)(row % g.Y), (int)(i - row * g.W));
#pragma unroll
        for (int d = 0; d < 6; d++) c += __popcll(f.e[d]);
    }
    bv_chunk_sum(c, counts);
}

// workgroup 0: the vertex chunks, workgroup 1: the quad chunks.  bv_scan_chunks with 64-bit sums (the int32 offsets
// are meaningless once a total reaches 2^31, which the totals tell), totals[blockIdx.x] = the sum.
__global__ __launch_bounds__(BV_SCAN_THREADS) void mh_scan_kernel(int* __restrict__ vcounts, int vchunks,
                                                                  int* __restrict__ qcounts, int qchunks,
                                                                  long long* __restrict__ totals) {
    __shared__ long long s_sum[BV_SCAN_THREADS];
    const long long sum = bv_scan_chunks(blockIdx.x == 0 ? vcounts : qcounts, blockIdx.x == 0 ? vchunks : qchunks, s_sum);
    if (threadIdx.x == BV_SCAN_THREADS - 1) totals[blockIdx.x] = sum;
}

__global__ __launch_bounds__(MH_CHUNK) void mh_prefix_kernel(const mh_u64* __restrict__ flags, int64_t fwords,
                                                             const int* __restrict__ offsets, int* __restrict__ prefix) {
    const int64_t i = (int64_t)blockIdx.x * MH_CHUNK + threadIdx.x;
    const int rank = bv_chunk_rank(i < fwords ? __popcll(flags[i]) : 0);
    if (i < fwords) prefix[i] = offsets[blockIdx.x] + rank;
}

// flag word and prefix of corner row (i, j), word cw; (0, 0) outside the lattice
__device__ __forceinline__ void mh_corner_word(const mh_u64* __restrict__ flags, const int* __restrict__ prefix,
                                               const mh_dims& g, int i, int j, int cw, mh_u64& f, int& p) {
    f = 0ull;
    p = 0;
    if ((unsigned)i > (unsigned)g.X || (unsigned)j > (unsigned)g.Y || (unsigned)cw >= (unsigned)g.CW) return;
    const int64_t at = ((int64_t)i * (g.Y + 1) + j) * g.CW + cw;
    f = flags[at];
    p = prefix[at];
}

__global__ __launch_bounds__(MH_CHUNK) void mh_vertex_kernel(const mh_u64* __restrict__ bits, mh_dims g,
                                                             const mh_u64* __restrict__ flags,
                                                             const int* __restrict__ prefix, int* __restrict__ corners,
                                                             int* __restrict__ neighbours, long long vcap) {
    const int64_t at = (int64_t)blockIdx.x * MH_CHUNK + threadIdx.x;
    if (at >= g.fwords) return;
    mh_u64 f = flags[at];
    if (!f) return;
    const int64_t row = at / g.CW;
    const int i = (int)(row / (g.Y + 1)), j = (int)(row % (g.Y + 1)), cw = (int)(at - row * g.CW);
    const mh_rows v = mh_load_rows(bits, g, i, j, cw);
    // the lattice edges leaving the corners of this word, per direction
    mh_u64 edge[6];
    edge[0] = mh_mixed2(v, 0, 1);                                           // voxels x = i - 1: rows (i-1, j-1), (i-1, j)
    edge[1] = mh_mixed2(v, 2, 3);
    edge[2] = mh_mixed2(v, 0, 2);                                           // voxels y = j - 1
    edge[3] = mh_mixed2(v, 1, 3);
    edge[4] = mh_mixed4(v.s);                                               // voxels z = k - 1
    edge[5] = mh_mixed4(v.r);
    mh_u64 nf[4];
    int np[4];
    mh_corner_word(flags, prefix, g, i - 1, j, cw, nf[0], np[0]);
    mh_corner_word(flags, prefix, g, i + 1, j, cw, nf[1], np[1]);
    mh_corner_word(flags, prefix, g, i, j - 1, cw, nf[2], np[2]);
    mh_corner_word(flags, prefix, g, i, j + 1, cw, nf[3], np[3]);
    long long rank = prefix[at];
    while (f) {                                                             // at most 64 trips: one per vertex
        const int b = __ffsll(f) - 1;
        f &= f - 1;
        if ((unsigned long long)rank < (unsigned long long)vcap) {
            const mh_u64 bit = 1ull << b, low = mh_below(b);
            int* c = corners + 3 * rank;
            c[0] = i;
            c[1] = j;
            c[2] = 64 * cw + b;
            int* n = neighbours + 6 * rank;
#pragma unroll
            for (int d = 0; d < 4; d++) n[d] = (edge[d] & bit) ? np[d] + __popcll(nf[d] & low) : -1;
            n[4] = (edge[4] & bit) ? (int)rank - 1 : -1;
            n[5] = (edge[5] & bit) ? (int)rank + 1 : -1;
        }
        rank++;
    }
}

// the corners q0 .. q3 of the quad of direction d as dx * 4 + dy * 2 + dz (the contract's table, written out)
__device__ static constexpr unsigned char MH_QUAD[6][4] = {
    {0, 1, 3, 2},                                                           // -x: (v, w) = (y, z), offsets 00 01 11 10
    {4, 6, 7, 5},                                                           // +x: 00 10 11 01
    {0, 4, 5, 1},                                                           // -y: (v, w) = (z, x)
    {2, 3, 7, 6},                                                           // +y
    {0, 2, 6, 4},                                                           // -z: (v, w) = (x, y)
    {1, 5, 7, 3},                                                           // +z
};

__global__ __launch_bounds__(MH_CHUNK) void mh_quad_kernel(const mh_u64* __restrict__ bits, mh_dims g,
                                                           const mh_u64* __restrict__ flags,
                                                           const int* __restrict__ prefix,
                                                           const int* __restrict__ offsets, int* __restrict__ faces,
                                                           long long qcap) {
    const int64_t at = (int64_t)blockIdx.x * MH_CHUNK + threadIdx.x;
    mh_faces f;
    int x = 0, y = 0, w = 0, c = 0;
#pragma unroll
    for (int d = 0; d < 6; d++) f.e[d] = 0ull;
    if (at < g.mwords) {
        const int64_t row = at / g.W;
        x = (int)(row / g.Y), y = (int)(row % g.Y), w = (int)(at - row * g.W);
        f = mh_exposed(bits, g, x, y, w);
#pragma unroll
        for (int d = 0; d < 6; d++) c += __popcll(f.e[d]);
    }
    long long rank = (long long)offsets[blockIdx.x] + bv_chunk_rank(c);
    if (!c) return;
    // flag words and prefixes of the voxel row's four corner rows: word w holds the corners k = z of this word's
    // voxels and all of k = z + 1 but the last, which is bit 0 of word w + 1
    mh_u64 cf[4][2];
    int cp[4][2];
#pragma unroll
    for (int n = 0; n < 4; n++) {
        mh_corner_word(flags, prefix, g, x + (n >> 1), y + (n & 1), w, cf[n][0], cp[n][0]);
        mh_corner_word(flags, prefix, g, x + (n >> 1), y + (n & 1), w + 1, cf[n][1], cp[n][1]);
    }
    mh_u64 any = f.e[0] | f.e[1] | f.e[2] | f.e[3] | f.e[4] | f.e[5];
    while (any) {                                                           // at most 64 trips: one per surface voxel
        const int b = __ffsll(any) - 1;
        any &= any - 1;
        int id[8];
#pragma unroll
        for (int n = 0; n < 4; n++) {
            id[2 * n] = cp[n][0] + __popcll(cf[n][0] & mh_below(b));
            id[2 * n + 1] = b < 63 ? cp[n][0] + __popcll(cf[n][0] & mh_below(b + 1)) : cp[n][1];
        }
#pragma unroll
        for (int d = 0; d < 6; d++) {
            if (!(f.e[d] >> b & 1ull)) continue;
            if ((unsigned long long)rank < (unsigned long long)qcap) {
                int* t = faces + 6 * rank;
                const int q0 = id[MH_QUAD[d][0]], q1 = id[MH_QUAD[d][1]], q2 = id[MH_QUAD[d][2]], q3 = id[MH_QUAD[d][3]];
                t[0] = q0;
                t[1] = q1;
                t[2] = q2;
                t[3] = q0;
                t[4] = q2;
                t[5] = q3;
            }
            rank++;
        }
    }
}

// ------------------------------------------------------------------------------------------------ smoothing
__global__ __launch_bounds__(256) void mh_smooth_kernel(const double* __restrict__ src, double* __restrict__ dst,
                                                        const int* __restrict__ neighbours, long long V, double factor) {
    for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < V; v += (long long)gridDim.x * 256) {
        const double px = src[3 * v], py = src[3 * v + 1], pz = src[3 * v + 2];
        double sx = 0.0, sy = 0.0, sz = 0.0;
        int m = 0;
#pragma unroll
        for (int d = 0; d < 6; d++) {
            const int n = neighbours[6 * v + d];
            if ((unsigned long long)n < (unsigned long long)V) {            // -1 (and anything out of range): absent
                sx = sx + src[3 * (long long)n];
                sy = sy + src[3 * (long long)n + 1];
                sz = sz + src[3 * (long long)n + 2];
                m++;
            }
        }
        double qx = px, qy = py, qz = pz;
        if (m) {
            const double dm = (double)m;
            qx = px + factor * (sx / dm - px);
            qy = py + factor * (sy / dm - py);
            qz = pz + factor * (sz / dm - pz);
        }
        dst[3 * v] = qx;
        dst[3 * v + 1] = qy;
        dst[3 * v + 2] = qz;
    }
}

// ------------------------------------------------------------------------------------------------ measures
struct mh_sums {
    double cross, triple;
};
__device__ __forceinline__ mh_sums mh_join(const mh_sums& a, const mh_sums& b) {
    mh_sums r = {a.cross + b.cross, a.triple + b.triple};
    return r;
}
// the workgroup's total in thread 0, in bv_block_join's fixed order
__device__ __forceinline__ mh_sums mh_block_join(mh_sums v, mh_sums* s_part) {
    return bv_block_join(v, s_part, [](const mh_sums& a, const mh_sums& b) { return mh_join(a, b); });
}

__global__ __launch_bounds__(MH_RTHREADS) void mh_measure_partial_kernel(const double* __restrict__ vertices, long long V,
                                                                         const int* __restrict__ faces, long long F,
                                                                         double* __restrict__ partial) {
    __shared__ mh_sums s_part[MH_RTHREADS / 64];
    const long long chunks = (F + MH_RCHUNK - 1) / MH_RCHUNK;
    for (long long chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
        mh_sums v = {0.0, 0.0};
#pragma unroll
        for (int k = 0; k < MH_RCHUNK / MH_RTHREADS; k++) {
            const long long t = chunk * MH_RCHUNK + k * MH_RTHREADS + threadIdx.x;
            if (t < F) {
                const long long a = faces[3 * t], b = faces[3 * t + 1], c = faces[3 * t + 2];
                if ((unsigned long long)a < (unsigned long long)V && (unsigned long long)b < (unsigned long long)V &&
                    (unsigned long long)c < (unsigned long long)V) {       // a face naming no vertex adds nothing
                    const double ax = vertices[3 * a], ay = vertices[3 * a + 1], az = vertices[3 * a + 2];
                    const double bx = vertices[3 * b], by = vertices[3 * b + 1], bz = vertices[3 * b + 2];
                    const double cx = vertices[3 * c], cy = vertices[3 * c + 1], cz = vertices[3 * c + 2];
                    const double ux = bx - ax, uy = by - ay, uz = bz - az, wx = cx - ax, wy = cy - ay, wz = cz - az;
                    const double nx = uy * wz - uz * wy, ny = uz * wx - ux * wz, nz = ux * wy - uy * wx;
                    v.cross += sqrt(nx * nx + ny * ny + nz * nz);
                    const double tx = by * cz - bz * cy, ty = bz * cx - bx * cz, tz = bx * cy - by * cx;
                    v.triple += ax * tx + ay * ty + az * tz;
                }
            }
        }
        v = mh_block_join(v, s_part);
        if (threadIdx.x == 0) {
            partial[2 * chunk] = v.cross;
            partial[2 * chunk + 1] = v.triple;
        }
    }
}

__global__ __launch_bounds__(MH_RTHREADS) void mh_measure_final_kernel(const double* __restrict__ partial, long long F,
                                                                       double* __restrict__ out) {
    __shared__ mh_sums s_part[MH_RTHREADS / 64];
    const long long chunks = (F + MH_RCHUNK - 1) / MH_RCHUNK;
    mh_sums v = {0.0, 0.0};
    for (long long chunk = threadIdx.x; chunk < chunks; chunk += MH_RTHREADS) {
        mh_sums w = {partial[2 * chunk], partial[2 * chunk + 1]};
        v = mh_join(v, w);
    }
    v = mh_block_join(v, s_part);
    if (threadIdx.x == 0) {
        out[0] = 0.5 * v.cross;
        out[1] = v.triple / 6.0;
    }
}

// ------------------------------------------------------------------------------------------------ host side
static inline mh_dims mh_make_dims(int X, int Y, int Z) {
    mh_dims g;
    g.X = X, g.Y = Y, g.Z = Z, g.W = bv_words(Z), g.CW = Z / 64 + 1;
    g.mwords = (int64_t)X * Y * g.W;
    g.fwords = ((int64_t)X + 1) * ((int64_t)Y + 1) * g.CW;
    g.tail = bv_tail(Z);
    return g;
}
// the workspace: flag words | int32 prefix per flag word | vertex chunk counts | quad chunk counts
struct mh_layout {
    size_t flags, prefix, vcounts, qcounts, total;
    int vchunks, qchunks;
};
static inline mh_layout mh_make_layout(const mh_dims& g) {
    mh_layout l;
    l.vchunks = (int)((g.fwords + MH_CHUNK - 1) / MH_CHUNK);
    l.qchunks = (int)((g.mwords + MH_CHUNK - 1) / MH_CHUNK);
    l.flags = 0;
    l.prefix = l.flags + bv_align((size_t)g.fwords * sizeof(mh_u64));
    l.vcounts = l.prefix + bv_align((size_t)g.fwords * sizeof(int));
    l.qcounts = l.vcounts + bv_align((size_t)l.vchunks * sizeof(int));
    l.total = l.qcounts + bv_align((size_t)l.qchunks * sizeof(int));
    return l;
}

extern "C" size_t ru3d_mesh_workspace_bytes(int X, int Y, int Z) {
    if (!bv_shape_ok(X, Y, Z)) return 0;
    return mh_make_layout(mh_make_dims(X, Y, Z)).total;
}

// flags, chunk counts, their scans and the two totals: the first half of both entry points
static void mh_launch_count(const mh_u64* bits, const mh_dims& g, const mh_layout& l, char* ws, long long* counts,
                            hipStream_t st) {
    hipLaunchKernelGGL(mh_flag_kernel, dim3(l.vchunks), dim3(MH_CHUNK), 0, st, bits, g, (mh_u64*)(ws + l.flags),
                       (int*)(ws + l.vcounts));
    hipLaunchKernelGGL(mh_quad_count_kernel, dim3(l.qchunks), dim3(MH_CHUNK), 0, st, bits, g, (int*)(ws + l.qcounts));
    hipLaunchKernelGGL(mh_scan_kernel, dim3(2), dim3(BV_SCAN_THREADS), 0, st, (int*)(ws + l.vcounts), l.vchunks,
                       (int*)(ws + l.qcounts), l.qchunks, counts);
}

extern "C" int ru3d_mesh_count(const uint64_t* bits, int X, int Y, int Z, int64_t* counts, void* ws, size_t ws_bytes,
                               void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    BV_REQUIRE_SHAPE("mesh_count");
    RU3D_REQUIRE(bits && counts && ws, "mesh_count: bad argument (null pointer)");
    const mh_dims g = mh_make_dims(X, Y, Z);
    const mh_layout l = mh_make_layout(g);
    RU3D_REQUIRE(ws_bytes >= l.total, "mesh_count: workspace of %zu bytes, %zu needed", ws_bytes, l.total);
    mh_launch_count((const mh_u64*)bits, g, l, (char*)ws, (long long*)counts, as_stream(stream));
    return ru3d_check_launch("mesh_count");
}

extern "C" int ru3d_mesh_emit(const uint64_t* bits, int X, int Y, int Z, int32_t* corners, int32_t* neighbours,
                              int64_t vcap, int32_t* faces, int64_t qcap, int64_t* counts, void* ws, size_t ws_bytes,
                              void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    BV_REQUIRE_SHAPE("mesh_emit");
    RU3D_REQUIRE(vcap >= 0 && vcap < ((int64_t)1 << 31), "mesh_emit: vertex capacity %lld (0 .. 2^31 - 1)",
                 (long long)vcap);
    RU3D_REQUIRE(qcap >= 0 && qcap < ((int64_t)1 << 30), "mesh_emit: quad capacity %lld (0 .. 2^30 - 1: two triangles a "
                 "quad, fewer than 2^31 triangles)", (long long)qcap);
    RU3D_REQUIRE(bits && counts && ws && (vcap == 0 || (corners && neighbours)) && (qcap == 0 || faces),
                 "mesh_emit: bad argument (null pointer)");
    const mh_dims g = mh_make_dims(X, Y, Z);
    const mh_layout l = mh_make_layout(g);
    RU3D_REQUIRE(ws_bytes >= l.total, "mesh_emit: workspace of %zu bytes, %zu needed", ws_bytes, l.total);
    hipStream_t st = as_stream(stream);
    char* w = (char*)ws;
    mh_launch_count((const mh_u64*)bits, g, l, w, (long long*)counts, st);
    if (vcap > 0 || qcap > 0)
        hipLaunchKernelGGL(mh_prefix_kernel, dim3(l.vchunks), dim3(MH_CHUNK), 0, st, (const mh_u64*)(w + l.flags), g.fwords,
                           (const int*)(w + l.vcounts), (int*)(w + l.prefix));
    if (vcap > 0)
        hipLaunchKernelGGL(mh_vertex_kernel, dim3(l.vchunks), dim3(MH_CHUNK), 0, st, (const mh_u64*)bits, g,
                           (const mh_u64*)(w + l.flags), (const int*)(w + l.prefix), (int*)corners, (int*)neighbours,
                           (long long)vcap);
    if (qcap > 0)
        hipLaunchKernelGGL(mh_quad_kernel, dim3(l.qchunks), dim3(MH_CHUNK), 0, st, (const mh_u64*)bits, g,
                           (const mh_u64*)(w + l.flags), (const int*)(w + l.prefix), (const int*)(w + l.qcounts),
                           (int*)faces, (long long)qcap);
    return ru3d_check_launch("mesh_emit");
}

extern "C" int ru3d_mesh_smooth(const double* src, double* dst, const int32_t* neighbours, int64_t V, double factor,
                                void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    RU3D_REQUIRE(V >= 1 && V < ((int64_t)1 << 31), "mesh_smooth: %lld vertices (1 .. 2^31 - 1)", (long long)V);
    RU3D_REQUIRE(src && dst && neighbours, "mesh_smooth: bad argument (null pointer)");
    RU3D_REQUIRE(src != dst, "mesh_smooth: not an in-place operation (src == dst)");
    RU3D_REQUIRE(isfinite(factor), "mesh_smooth: factor %g (finite)", factor);
    const int64_t cap = (int64_t)ru3d_get_cu_budget() * 8;
    int64_t blocks = (V + 255) / 256;
    blocks = blocks > cap ? cap : blocks;
    hipLaunchKernelGGL(mh_smooth_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), src, dst,
                       (const int*)neighbours, (long long)V, factor);
    return ru3d_check_launch("mesh_smooth");
}

extern "C" size_t ru3d_mesh_measure_workspace_bytes(int64_t F) {
    if (F < 1 || F >= ((int64_t)1 << 31)) return 0;
    return bv_align((size_t)((F + MH_RCHUNK - 1) / MH_RCHUNK) * 2 * sizeof(double));
}

extern "C" int ru3d_mesh_measure(const double* vertices, int64_t V, const int32_t* faces, int64_t F, double* out, void* ws,
                                 size_t ws_bytes, void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    RU3D_REQUIRE(V >= 1 && V < ((int64_t)1 << 31), "mesh_measure: %lld vertices (1 .. 2^31 - 1)", (long long)V);
    RU3D_REQUIRE(F >= 1 && F < ((int64_t)1 << 31), "mesh_measure: %lld faces (1 .. 2^31 - 1)", (long long)F);
    RU3D_REQUIRE(vertices && faces && out && ws, "mesh_measure: bad argument (null pointer)");
    RU3D_REQUIRE(ws_bytes >= ru3d_mesh_measure_workspace_bytes(F), "mesh_measure: workspace of %zu bytes, %zu needed",
                 ws_bytes, ru3d_mesh_measure_workspace_bytes(F));
    hipStream_t st = as_stream(stream);
    const int64_t chunks = (F + MH_RCHUNK - 1) / MH_RCHUNK, cap = (int64_t)ru3d_get_cu_budget() * 8;
    hipLaunchKernelGGL(mh_measure_partial_kernel, dim3((unsigned)(chunks < cap ? chunks : cap)), dim3(MH_RTHREADS), 0, st,
                       vertices, (long long)V, (const int*)faces, (long long)F, (double*)ws);
    hipLaunchKernelGGL(mh_measure_final_kernel, dim3(1), dim3(MH_RTHREADS), 0, st, (const double*)ws, (long long)F, out);
    return ru3d_check_launch("mesh_measure");
}
