// The voxel graph of a packed mask (a curve skeleton, but any mask will do): nodes, branches, what is measured per node
// and per branch, and the erasure of chosen nodes and branches.  The contract is written down in include/ru3d.h
// ("skeleton graph"); the numpy twin that defines the result is transform._skeleton_graph_numpy.
//
// There is no list of voxels and no dense volume of labels.  The set voxels are addressed by their rank in element
// order: rank(p) = prefix[word of p] + popcount(the set bits of that word below p), with one int of exclusive popcount
// prefix per 64-voxel word (the three-launch compaction of bitvol.h, 256 words to a chunk).  A second bit volume marks
// the path voxels (exactly two set voxels among the 26 neighbours, the bit-sliced counter of sk_classify_kernel), so the
// kind of any neighbour is one bit test.  A thread owns a word: it holds the 3 x 3 rows of three words around it in
// registers and walks the set bits of its word.
//   sg_kind_kernel      path bits of every word, set voxels per chunk
//   sg_scan_kernel      chunk counts -> exclusive prefix sums, the total
//   sg_prefix_kernel    prefix per word; ids[r] = the rank at which r's run of like voxels along z begins in its word
//   sg_union_kernel     union-find on ids over the 13 forward offsets, linking like with like only.  parent <= child
//                       always, so a component's root is its smallest rank = its first voxel.  As in components.hip, ids
//                       is read with agent-scope relaxed atomic loads, a decision rests only on what an atomicMin
//                       returned, and every step goes to a strictly smaller rank or stops: a stale parent is still an
//                       ancestor and costs a retry, never a wrong union, and nobody waits for anybody.  sg_find halves
//                       the path it walks (atomicMin of a voxel's parent with its grandparent).
//   sg_flatten_kernel   ids[r] = find(r); a bit volume of the roots; node roots and branch roots per chunk
//   sg_scan2_kernel     both kinds of chunk counts -> prefix sums, M and B
//   sg_number_kernel    roots in rank order receive -m / +b
//   sg_finalize_kernel  everything else reads its root's number (this launch writes no root and reads nothing else)
//   sg_measure_*        init, one pass of integer atomics (runs of one id inside a word are summed in registers first),
//                       and the unpacking of the terminals: (linear index << 32 | node) under atomicMin / atomicMax gives
//                       (t0, n0) and (t1, n1) in the order the contract asks for.
//   sg_erase_kernel     a thread clears the flagged voxels of its own word
// Visibility between the steps comes from the kernel boundaries.  Integer atomics only, no floating-point addition: two
// runs give identical bytes under every grid.
#include <limits.h>
#include <math.h>
#include "common.h"
#include "bitvol.h"

#pragma clang fp contract(off)

typedef unsigned long long sg_u64;

#define SG_CHUNK BV_CHUNK_THREADS          // words of a chunk = threads of its workgroup
#define SG_COUNTERS 256                    // bytes of counters at the head of the workspace
#define SG_N26 0x7ffdfffu                  // the 27-bit neighbourhood code of skeleton.hip without the voxel itself
#define SG_FWD 0x7ffc000u                  // cells 14 .. 26: the 13 offsets towards larger linear indices
#define SG_NODE_COLS 6
#define SG_BRANCH_COLS 18
#define SG_RADII_COLS 3

struct sg_geom {
    int X, Y, Z, W;
    sg_u64 tail;
    int64_t words;
};

// the scratch of one call: sections of the caller's workspace
struct sg_scratch {
    long long* total;                      // set voxels (measure and erase; label counts into the caller's counts[0])
    int* cnt_a;                            // per chunk: set voxels, later node roots
    int* cnt_b;                            // per chunk: branch roots
    int* prefix;                           // per word
    sg_u64* path;                          // per word: the path voxels
    sg_u64* roots;                         // per word: the voxels that are the first of their node or branch
};

__device__ __forceinline__ int sg_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void sg_store(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// bits z - 1, z, z + 1 (z = 64 w + b) of the row whose words w - 1, w, w + 1 are prev, cur, next
__device__ __forceinline__ unsigned sg_three(sg_u64 prev, sg_u64 cur, sg_u64 next, int b) {
    unsigned t = b == 0 ? (unsigned)((cur << 1) | (prev >> 63)) : (unsigned)(cur >> (b - 1));
    if (b == 63) t |= (unsigned)(next & 1ull) << 2;
    return t & 7u;
}

__device__ __forceinline__ void sg_where(const sg_geom& g, int64_t i, int* x, int* y, int* w) {
    const int64_t row = i / g.W;
    *w = (int)(i - row * g.W);
    *y = (int)(row % g.Y);
    *x = (int)(row / g.Y);
}

// the rank of the set voxel (x, y, z), which lies inside the volume
__device__ __forceinline__ int sg_rank(const sg_u64* __restrict__ mask, const int* __restrict__ prefix, const sg_geom& g, int x,
                                       int y, int z) {
    const int w = z >> 6;
    const int64_t i = ((int64_t)x * g.Y + y) * g.W + w;
    const sg_u64 m = bv_word_masked(mask, g.X, g.Y, g.W, g.tail, x, y, w);
    return prefix[i] + __popcll(m & (((sg_u64)1 << (z & 63)) - 1));
}

// ------------------------------------------------------------------------------------------------ union-find
// Walks only to strictly smaller ranks: it ends on any memory contents.
__device__ __forceinline__ int sg_find(int* L, int a) {
    for (;;) {
        const int p = sg_load(L + a);
        if (p >= a) return a;
        const int gp = sg_load(L + p);
        if (gp >= p) return p;
        atomicMin(&L[a], gp);                       // an ancestor of a: the sets stay what they are
        a = gp;
    }
}
__device__ __forceinline__ void sg_unite(int* L, int a, int b) {
    for (;;) {
        a = sg_find(L, a);
        b = sg_find(L, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = atomicMin(&L[a], b);        // a was a root when this returns a: it now hangs under b
        if (old >= a) return;
        a = old;                                    // a had a parent already: that parent and b are still to be united
    }
}

// ------------------------------------------------------------------------------------------------ ranks and kinds
__global__ __launch_bounds__(SG_CHUNK) void sg_kind_kernel(const sg_u64* __restrict__ mask, const sg_geom g,
                                                           sg_u64* __restrict__ path, int* __restrict__ counts) {
    const int64_t i = (int64_t)blockIdx.x * SG_CHUNK + threadIdx.x;
    sg_u64 m = 0;
    if (i < g.words) {
        int x, y, w;
        sg_where(g, i, &x, &y, &w);
        m = bv_word_masked(mask, g.X, g.Y, g.W, g.tail, x, y, w);
        sg_u64 two = 0;
        if (m) {
            sg_u64 c0 = 0, c1 = 0, sat = 0;                                 // per voxel: count = c1 c0, or "4 or more"
#pragma unroll
            for (int r = 0; r < 9; r++) {
                const int nx = x + r / 3 - 1, ny = y + r % 3 - 1;
                const sg_u64 prev = bv_word_masked(mask, g.X, g.Y, g.W, g.tail, nx, ny, w - 1),
                             cur = bv_word_masked(mask, g.X, g.Y, g.W, g.tail, nx, ny, w),
                             next = bv_word_masked(mask, g.X, g.Y, g.W, g.tail, nx, ny, w + 1);
#pragma unroll
                for (int dz = -1; dz <= 1; dz++) {
                    if (r == 4 && dz == 0) continue;
                    const sg_u64 v = bv_zview(prev, cur, next, dz);
                    const sg_u64 carry = c0 & v;
                    c0 ^= v;
                    sat |= c1 & carry;
                    c1 ^= carry;
                }
            }
            two = m & ~c0 & c1 & ~sat;
        }
        path[i] = two;
    }
    bv_chunk_sum(__popcll(m), counts);
}

__global__ __launch_bounds__(BV_SCAN_THREADS) void sg_scan_kernel(int* __restrict__ counts, int chunks,
                                                                  long long* __restrict__ total) {
    __shared__ int s_sum[BV_SCAN_THREADS];
    const int sum = bv_scan_chunks(counts, chunks, s_sum);
    if (threadIdx.x == BV_SCAN_THREADS - 1) *total = (long long)sum;
}

// ids == NULL: the prefix alone
__global__ __launch_bounds__(SG_CHUNK) void sg_prefix_kernel(const sg_u64* __restrict__ mask, const sg_u64* __restrict__ path,
                                                             const sg_geom g, const int* __restrict__ offsets,
                                                             int* __restrict__ prefix, int* __restrict__ ids, long long capacity,
                                                             const long long* __restrict__ total) {
    const int64_t i = (int64_t)blockIdx.x * SG_CHUNK + threadIdx.x;
    sg_u64 m = 0;
    if (i < g.words) {
        int x, y, w;
        sg_where(g, i, &x, &y, &w);
        m = bv_word_masked(mask, g.X, g.Y, g.W, g.tail, x, y, w);
    }
    int pos = offsets[blockIdx.x] + bv_chunk_rank(__popcll(m));
    if (i >= g.words) return;
    prefix[i] = pos;
    if (!ids || *total > capacity || !m) return;
    const sg_u64 pm = path[i];
    int start = pos, last_b = -2, last_kind = 0;
    while (m) {                                                             // at most 64 trips: one per set bit
        const int b = __ffsll(m) - 1;
        m &= m - 1;
        const int kind = (int)((pm >> b) & 1ull);
        if (b != last_b + 1 || kind != last_kind) start = pos;              // a new run of like voxels along z
        ids[pos] = start;
        last_b = b;
        last_kind = kind;
        pos++;
    }
}

// ------------------------------------------------------------------------------------------------ labelling
__global__ __launch_bounds__(256) void sg_union_kernel(const sg_u64* __restrict__ mask, const sg_u64* __restrict__ path,
                                                       const int* __restrict__ prefix, const sg_geom g, int* ids,
                                                       long long capacity, const long long* __restrict__ total) {
    if (*total > capacity) return;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < g.words; i += (int64_t)gridDim.x * 256) {
        int x, y, w;
        sg_where(g, i, &x, &y, &w);
        sg_u64 m = bv_word_masked(mask, g.X, g.Y, g.W, g.tail, x, y, w);
        if (!m) continue;
        sg_u64 rows[5][3], prows[5][3];                                     // the rows (0, 0), (0, 1), (1, -1), (1, 0), (1, 1)
#pragma unroll
        for (int r = 4; r < 9; r++) {
            const int nx = x + r / 3 - 1, ny = y + r % 3 - 1;
#pragma unroll
            for (int k = 0; k < 3; k++) {
                rows[r - 4][k] = bv_word_masked(mask, g.X, g.Y, g.W, g.tail, nx, ny, w - 1 + k);
                prows[r - 4][k] = bv_word(path, g.X, g.Y, g.W, nx, ny, w - 1 + k);
            }
        }
        int pos = prefix[i];
        while (m) {
            const int b = __ffsll(m) - 1;
            m &= m - 1;
            unsigned code = 0, pcode = 0;
#pragma unroll
            for (int r = 4; r < 9; r++) {
                code |= sg_three(rows[r - 4][0], rows[r - 4][1], rows[r - 4][2], b) << (3 * r);
                pcode |= sg_three(prows[r - 4][0], prows[r - 4][1], prows[r - 4][2], b) << (3 * r);
            }
            unsigned like = code & SG_FWD & (((pcode >> 13) & 1u) ? pcode : ~pcode);
            if (b < 63) like &= ~(1u << 14);                                // z + 1 in this word: sg_prefix_kernel's run
            while (like) {
                const int c = __ffs(like) - 1;
                like &= like - 1;
                const int q = sg_rank(mask, prefix, g, x + c / 9 - 1, y + (c / 3) % 3 - 1, 64 * w + b + c % 3 - 1);
                sg_unite(ids, pos, q);
            }
            pos++;
        }
    }
}

// counts[chunk] = node roots + (branch roots << 16): a chunk holds 2^14 voxels
__global__ __launch_bounds__(SG_CHUNK) void sg_flatten_kernel(const sg_u64* __restrict__ mask, const sg_u64* __restrict__ path,
                                                              const int* __restrict__ prefix, const sg_geom g, int* ids,
                                                              long long capacity, const long long* __restrict__ total,
                                                              sg_u64* __restrict__ roots, int* __restrict__ counts) {
    const int64_t i = (int64_t)blockIdx.x * SG_CHUNK + threadIdx.x;
    int c = 0;
    if (i < g.words) {
        sg_u64 rb = 0;
        if (*total <= capacity) {
            int x, y, w;
            sg_where(g, i, &x, &y, &w);
            sg_u64 m = bv_word_masked(mask, g.X, g.Y, g.W, g.tail, x, y, w);
            const sg_u64 pm = path[i];
            int pos = prefix[i];
            while (m) {
                const int b = __ffsll(m) - 1;
                m &= m - 1;
                const int r = sg_find(ids, pos);
                if (r != pos) {
                    sg_store(ids + pos, r);
                } else {
                    rb |= (sg_u64)1 << b;
                    c += ((pm >> b) & 1ull) ? 0x10000 : 1;
                }
                pos++;
            }
        }
        roots[i] = rb;
    }
    bv_chunk_sum(c, counts);
}

__global__ __launch_bounds__(BV_SCAN_THREADS) void sg_scan2_kernel(int* __restrict__ cnt_a, int* __restrict__ cnt_b, int chunks,
                                                                   long long* __restrict__ counts) {
    __shared__ int s_sum[BV_SCAN_THREADS];
    const int per = (chunks + BV_SCAN_THREADS - 1) / BV_SCAN_THREADS;       // the counts bv_scan_chunks gives this thread
    const int lo = min(chunks, (int)threadIdx.x * per), hi = min(chunks, lo + per);
    for (int k = lo; k < hi; k++) {
        const int v = cnt_a[k];
        cnt_a[k] = v & 0xffff;
        cnt_b[k] = v >> 16;
    }
    const int M = bv_scan_chunks(cnt_a, chunks, s_sum);
    __syncthreads();
    const int B = bv_scan_chunks(cnt_b, chunks, s_sum);
    if (threadIdx.x == BV_SCAN_THREADS - 1) {
        counts[1] = M;
        counts[2] = B;
    }
}

__global__ __launch_bounds__(SG_CHUNK) void sg_number_kernel(const sg_u64* __restrict__ mask, const sg_u64* __restrict__ path,
                                                             const sg_u64* __restrict__ roots, const int* __restrict__ prefix,
                                                             const sg_geom g, const int* __restrict__ off_nodes,
                                                             const int* __restrict__ off_branches, int* __restrict__ ids,
                                                             long long capacity, const long long* __restrict__ total) {
    const int64_t i = (int64_t)blockIdx.x * SG_CHUNK + threadIdx.x;
    sg_u64 rb = 0, pm = 0;
    if (i < g.words) {
        rb = roots[i];
        pm = path[i];
    }
    const int rank = bv_chunk_rank(__popcll(rb & ~pm) | (__popcll(rb & pm) << 16));
    if (!rb || *total > capacity) return;
    int node = off_nodes[blockIdx.x] + (rank & 0xffff), branch = off_branches[blockIdx.x] + (rank >> 16);
    int x, y, w;
    sg_where(g, i, &x, &y, &w);
    const sg_u64 m = bv_word_masked(mask, g.X, g.Y, g.W, g.tail, x, y, w);
    const int base = prefix[i];
    while (rb) {
        const int b = __ffsll(rb) - 1;
        rb &= rb - 1;
        const int pos = base + __popcll(m & (((sg_u64)1 << b) - 1));
        ids[pos] = ((pm >> b) & 1ull) ? ++branch : -(++node);
    }
}

__global__ __launch_bounds__(256) void sg_finalize_kernel(const sg_u64* __restrict__ mask, const sg_u64* __restrict__ roots,
                                                          const int* __restrict__ prefix, const sg_geom g, int* ids,
                                                          long long capacity, const long long* __restrict__ total) {
    if (*total > capacity) return;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < g.words; i += (int64_t)gridDim.x * 256) {
        int x, y, w;
        sg_where(g, i, &x, &y, &w);
        const sg_u64 m = bv_word_masked(mask, g.X, g.Y, g.W, g.tail, x, y, w);
        sg_u64 rest = m & ~roots[i];
        const int base = prefix[i];
        while (rest) {
            const int b = __ffsll(rest) - 1;
            rest &= rest - 1;
            const int pos = base + __popcll(m & (((sg_u64)1 << b) - 1));
            ids[pos] = ids[ids[pos]];                                       // its root's number: roots are not written here
        }
    }
}

// ------------------------------------------------------------------------------------------------ measurements
__global__ __launch_bounds__(256) void sg_measure_init_kernel(long long* __restrict__ nodes, long long M,
                                                              long long* __restrict__ branches, long long* __restrict__ radii,
                                                              long long B) {
    const long long step = (long long)gridDim.x * 256, at = (long long)blockIdx.x * 256 + threadIdx.x;
    for (long long k = at; k < M * SG_NODE_COLS; k += step) nodes[k] = k % SG_NODE_COLS == 5 ? LLONG_MAX : 0;
    for (long long k = at; k < B * SG_BRANCH_COLS; k += step) branches[k] = k % SG_BRANCH_COLS == 1 ? -1ll : 0;     // all ones
    if (radii)
        for (long long k = at; k < B * SG_RADII_COLS; k += step)
            radii[k] = k % SG_RADII_COLS == 0 ? 0x7ff0000000000000ll : 0;                   // min: +inf, max: 0.0, sum: 0
}

// what a thread has summed for the run of one id it is in
struct sg_run {
    int id, voxels, valence, first;
    long long sum_z;
};

__device__ __forceinline__ void sg_flush(const sg_run& r, int x, int y, long long* __restrict__ nodes,
                                         long long* __restrict__ branches) {
    if (r.id < 0) {
        sg_u64* row = (sg_u64*)(nodes + (long long)(-r.id - 1) * SG_NODE_COLS);
        atomicAdd(row + 0, (sg_u64)r.voxels);
        if (r.valence) atomicAdd(row + 1, (sg_u64)r.valence);
        atomicAdd(row + 2, (sg_u64)((long long)r.voxels * x));
        atomicAdd(row + 3, (sg_u64)((long long)r.voxels * y));
        atomicAdd(row + 4, (sg_u64)r.sum_z);
        atomicMin(row + 5, (sg_u64)r.first);
    } else if (r.id > 0) {
        atomicAdd((sg_u64*)(branches + (long long)(r.id - 1) * SG_BRANCH_COLS), (sg_u64)r.voxels);
    }
}

__global__ __launch_bounds__(256) void sg_measure_kernel(const sg_u64* __restrict__ mask, const sg_u64* __restrict__ path,
                                                         const int* __restrict__ prefix, const sg_geom g,
                                                         const int* __restrict__ ids, long long n, long long M, long long B,
                                                         const double* __restrict__ sq, long long* __restrict__ nodes,
                                                         long long* __restrict__ branches, long long* __restrict__ radii) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < g.words; i += (int64_t)gridDim.x * 256) {
        int x, y, w;
        sg_where(g, i, &x, &y, &w);
        sg_u64 m = bv_word_masked(mask, g.X, g.Y, g.W, g.tail, x, y, w);
        if (!m) continue;
        sg_u64 rows[9][3], prows[9][3];
#pragma unroll
        for (int r = 0; r < 9; r++) {
            const int nx = x + r / 3 - 1, ny = y + r % 3 - 1;
#pragma unroll
            for (int k = 0; k < 3; k++) {
                rows[r][k] = bv_word_masked(mask, g.X, g.Y, g.W, g.tail, nx, ny, w - 1 + k);
                prows[r][k] = bv_word(path, g.X, g.Y, g.W, nx, ny, w - 1 + k);
            }
        }
        const int64_t row0 = (i / g.W) * g.Z;                               // the linear index of (x, y, 0)
        int pos = prefix[i];
        sg_run run = {0, 0, 0, 0, 0};
        while (m && pos < n) {                                              // ranks beyond n: not the mask that was labelled
            const int b = __ffsll(m) - 1;
            m &= m - 1;
            const int z = 64 * w + b, lin = (int)(row0 + z);
            int id = ids[pos++];
            if (id < -M || id > B) id = 0;
            if (id != run.id) {
                sg_flush(run, x, y, nodes, branches);
                run.id = id;
                run.voxels = run.valence = 0;
                run.sum_z = 0;
                run.first = lin;
            }
            if (!id) continue;
            unsigned code = 0, pcode = 0;
#pragma unroll
            for (int r = 0; r < 9; r++) {
                code |= sg_three(rows[r][0], rows[r][1], rows[r][2], b) << (3 * r);
                pcode |= sg_three(prows[r][0], prows[r][1], prows[r][2], b) << (3 * r);
            }
            code &= SG_N26;
            run.voxels++;
            if (id < 0) {
                run.sum_z += z;
                run.valence += __popc(code & pcode);                        // a path voxel beside it: one attachment
                continue;
            }
            long long* row = branches + (long long)(id - 1) * SG_BRANCH_COLS;
            while (code) {                                                  // the two neighbours of a path voxel
                const int c = __ffs(code) - 1;
                code &= code - 1;
                if ((pcode >> c) & 1u) {                                    // the same branch: the lower voxel counts the pair
                    if (c > 13) atomicAdd((sg_u64*)(row + 5 + c - 14), 1ull);
                    continue;
                }
                atomicAdd((sg_u64*)(row + 5 + (c > 13 ? c - 14 : 12 - c)), 1ull);
                const int q = sg_rank(mask, prefix, g, x + c / 9 - 1, y + (c / 3) % 3 - 1, z + c % 3 - 1);
                if (q >= n) continue;
                const int node = -ids[q];
                if (node < 1 || node > M) continue;
                const sg_u64 key = (sg_u64)(unsigned)lin << 32 | (unsigned)node;
                atomicMin((sg_u64*)(row + 1), key);
                atomicMax((sg_u64*)(row + 2), key);
            }
            if (sq) {
                const double v = sq[lin];
                long long* rr = radii + (long long)(id - 1) * SG_RADII_COLS;
                atomicMin((sg_u64*)(rr + 0), (sg_u64)__double_as_longlong(v));      // v >= 0: the bit patterns order like the values
                atomicMax((sg_u64*)(rr + 1), (sg_u64)__double_as_longlong(v));
                if (isfinite(v)) atomicAdd((sg_u64*)(rr + 2), (sg_u64)llrint(sqrt(v) * 16777216.0));
            }
        }
        sg_flush(run, x, y, nodes, branches);
    }
}

// (t0 << 32 | n0), (t1 << 32 | n1) -> t0, t1, n0, n1; a loop was never touched
__global__ __launch_bounds__(256) void sg_measure_finish_kernel(long long* __restrict__ branches, long long B) {
    for (long long k = (long long)blockIdx.x * 256 + threadIdx.x; k < B; k += (long long)gridDim.x * 256) {
        long long* row = branches + k * SG_BRANCH_COLS;
        const sg_u64 lo = (sg_u64)row[1], hi = (sg_u64)row[2];
        const bool loop = hi == 0;
        row[1] = loop ? -1 : (long long)(lo >> 32);
        row[2] = loop ? -1 : (long long)(hi >> 32);
        row[3] = loop ? -1 : (long long)(lo & 0xffffffffull);
        row[4] = loop ? -1 : (long long)(hi & 0xffffffffull);
    }
}

// ------------------------------------------------------------------------------------------------ erasure
__global__ __launch_bounds__(256) void sg_erase_kernel(sg_u64* __restrict__ mask, const int* __restrict__ prefix, const sg_geom g,
                                                       const int* __restrict__ ids, long long n, long long M, long long B,
                                                       const uint8_t* __restrict__ flags_branch,
                                                       const uint8_t* __restrict__ flags_node) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < g.words; i += (int64_t)gridDim.x * 256) {
        int x, y, w;
        sg_where(g, i, &x, &y, &w);
        const sg_u64 m = bv_word_masked(mask, g.X, g.Y, g.W, g.tail, x, y, w);
        sg_u64 rest = m, kill = 0;
        int pos = prefix[i];
        while (rest && pos < n) {
            const int b = __ffsll(rest) - 1;
            rest &= rest - 1;
            const int id = ids[pos++];
            bool hit = false;
            if (id > 0 && id <= B) hit = flags_branch && flags_branch[id - 1];
            if (id < 0 && id >= -M) hit = flags_node && flags_node[-id - 1];
            if (hit) kill |= (sg_u64)1 << b;
        }
        if (kill) mask[i] = m & ~kill;
    }
}

// ------------------------------------------------------------------------------------------------ host side
static inline unsigned sg_blocks(int64_t items) {
    const int64_t cap = (int64_t)ru3d_get_cu_budget() * 8;
    int64_t blocks = (items + 255) / 256;
    blocks = blocks > cap ? cap : blocks;
    return (unsigned)(blocks < 1 ? 1 : blocks);
}

static inline sg_geom sg_geometry(int X, int Y, int Z) {
    sg_geom g = {X, Y, Z, bv_words(Z), bv_tail(Z), (int64_t)X * Y * bv_words(Z)};
    return g;
}

static inline int sg_chunks(const sg_geom& g) { return (int)((g.words + SG_CHUNK - 1) / SG_CHUNK); }

static inline sg_scratch sg_carve(void* ws, const sg_geom& g) {
    char* p = (char*)ws;
    sg_scratch s;
    s.total = (long long*)p;
    p += SG_COUNTERS;
    s.cnt_a = (int*)p;
    p += bv_align((size_t)sg_chunks(g) * sizeof(int));
    s.cnt_b = (int*)p;
    p += bv_align((size_t)sg_chunks(g) * sizeof(int));
    s.prefix = (int*)p;
    p += bv_align((size_t)g.words * sizeof(int));
    s.path = (sg_u64*)p;
    p += bv_align((size_t)g.words * sizeof(sg_u64));
    s.roots = (sg_u64*)p;
    return s;
}

// what sg_carve hands out
static size_t sg_carved_bytes(const sg_geom& g) {
    return SG_COUNTERS + 2 * bv_align((size_t)sg_chunks(g) * sizeof(int)) + bv_align((size_t)g.words * sizeof(int)) +
           2 * bv_align((size_t)g.words * sizeof(sg_u64));
}

// The workspace of the three entry points is three times that of the thinning: 768 bytes and three 64-bit planes of the
// packed words, each rounded up to 256 bytes.  The sections above are the counters, two planes, half a plane of prefix
// sums and two ints per 256 words: with A the rounding, w the words and c = ceil(w / 256), 2 A(4 c) <= 512 + A(8 w) -
// A(4 w) holds for every w (A(4 c) = 256 up to 16384 words, and beyond them 4 w - 256 outgrows w / 32 + 518).
static size_t sg_workspace_bytes(int X, int Y, int Z) { return 3 * ru3d_skeleton_workspace_bytes(X, Y, Z); }

#define SG_REQUIRE_WORKSPACE(what)                                                                                  \
    RU3D_REQUIRE(ws_bytes >= sg_workspace_bytes(X, Y, Z) &&                                                         \
                     sg_carved_bytes(sg_geometry(X, Y, Z)) <= sg_workspace_bytes(X, Y, Z),                          \
                 what ": workspace of %zu bytes, %zu needed", ws_bytes, sg_workspace_bytes(X, Y, Z))

// kinds, chunk sums, scan, prefix (and the run parents of ids, when there is one)
static void sg_prepare(const sg_u64* mask, const sg_geom& g, const sg_scratch& s, long long* total, int* ids, long long capacity,
                       hipStream_t st) {
    const int chunks = sg_chunks(g);
    hipLaunchKernelGGL(sg_kind_kernel, dim3(chunks), dim3(SG_CHUNK), 0, st, mask, g, s.path, s.cnt_a);
    hipLaunchKernelGGL(sg_scan_kernel, dim3(1), dim3(BV_SCAN_THREADS), 0, st, s.cnt_a, chunks, total);
    hipLaunchKernelGGL(sg_prefix_kernel, dim3(chunks), dim3(SG_CHUNK), 0, st, mask, (const sg_u64*)s.path, g,
                       (const int*)s.cnt_a, s.prefix, ids, capacity, (const long long*)total);
}

extern "C" int ru3d_skeleton_graph_label(const uint64_t* skel, int X, int Y, int Z, int32_t* ids, int64_t capacity,
                                         int64_t* counts, void* ws, size_t ws_bytes, void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    BV_REQUIRE_SHAPE("skeleton_graph_label");
    RU3D_REQUIRE(skel && counts && ws, "skeleton_graph_label: bad argument (null pointer)");
    RU3D_REQUIRE(ids ? capacity >= 1 : capacity == 0,
                 "skeleton_graph_label: capacity %lld (>= 1 with ids, 0 without)", (long long)capacity);
    SG_REQUIRE_WORKSPACE("skeleton_graph_label");
    hipStream_t st = as_stream(stream);
    const sg_geom g = sg_geometry(X, Y, Z);
    const sg_scratch s = sg_carve(ws, g);
    const int chunks = sg_chunks(g);
    const sg_u64* mask = (const sg_u64*)skel;
    long long* total = (long long*)counts;
    const long long cap = ids ? (long long)capacity : -1;                   // -1: nothing is labelled, M = B = 0
    sg_prepare(mask, g, s, total, (int*)ids, cap, st);
    if (ids) {
        hipLaunchKernelGGL(sg_union_kernel, dim3(sg_blocks(g.words)), dim3(256), 0, st, mask, (const sg_u64*)s.path,
                           (const int*)s.prefix, g, (int*)ids, cap, (const long long*)total);
    }
    hipLaunchKernelGGL(sg_flatten_kernel, dim3(chunks), dim3(SG_CHUNK), 0, st, mask, (const sg_u64*)s.path, (const int*)s.prefix,
                       g, (int*)ids, cap, (const long long*)total, s.roots, s.cnt_a);
    hipLaunchKernelGGL(sg_scan2_kernel, dim3(1), dim3(BV_SCAN_THREADS), 0, st, s.cnt_a, s.cnt_b, chunks, total);
    if (ids) {
        hipLaunchKernelGGL(sg_number_kernel, dim3(chunks), dim3(SG_CHUNK), 0, st, mask, (const sg_u64*)s.path,
                           (const sg_u64*)s.roots, (const int*)s.prefix, g, (const int*)s.cnt_a, (const int*)s.cnt_b, (int*)ids,
                           cap, (const long long*)total);
        hipLaunchKernelGGL(sg_finalize_kernel, dim3(sg_blocks(g.words)), dim3(256), 0, st, mask, (const sg_u64*)s.roots,
                           (const int*)s.prefix, g, (int*)ids, cap, (const long long*)total);
    }
    return ru3d_check_launch("skeleton_graph_label");
}

extern "C" int ru3d_skeleton_graph_measure(const uint64_t* skel, int X, int Y, int Z, const int32_t* ids, int64_t n, int64_t M,
                                           int64_t B, const double* sq, int64_t* nodes, int64_t* branches, void* branch_radii,
                                           void* ws, size_t ws_bytes, void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    BV_REQUIRE_SHAPE("skeleton_graph_measure");
    RU3D_REQUIRE(n >= 0 && M >= 0 && B >= 0 && M <= n && B <= n && n <= (int64_t)X * Y * Z,
                 "skeleton_graph_measure: %lld voxels, %lld nodes, %lld branches in %lld voxels of volume", (long long)n,
                 (long long)M, (long long)B, (long long)X * Y * Z);
    RU3D_REQUIRE(skel && ws && (ids || !n) && (nodes || !M) && (branches || !B),
                 "skeleton_graph_measure: bad argument (null pointer)");
    RU3D_REQUIRE(!sq == !branch_radii || (sq && !B), "skeleton_graph_measure: sq and branch_radii go together");
    SG_REQUIRE_WORKSPACE("skeleton_graph_measure");
    if (!n) return 0;
    hipStream_t st = as_stream(stream);
    const sg_geom g = sg_geometry(X, Y, Z);
    const sg_scratch s = sg_carve(ws, g);
    const sg_u64* mask = (const sg_u64*)skel;
    const bool with_radii = sq && branch_radii;
    sg_prepare(mask, g, s, s.total, nullptr, -1, st);
    const int64_t cells = M * SG_NODE_COLS > B * SG_BRANCH_COLS ? M * SG_NODE_COLS : B * SG_BRANCH_COLS;
    hipLaunchKernelGGL(sg_measure_init_kernel, dim3(sg_blocks(cells)), dim3(256), 0, st, (long long*)nodes, (long long)M,
                       (long long*)branches, with_radii ? (long long*)branch_radii : (long long*)nullptr, (long long)B);
    hipLaunchKernelGGL(sg_measure_kernel, dim3(sg_blocks(g.words)), dim3(256), 0, st, mask, (const sg_u64*)s.path,
                       (const int*)s.prefix, g, (const int*)ids, (long long)n, (long long)M, (long long)B,
                       with_radii ? sq : (const double*)nullptr, (long long*)nodes, (long long*)branches,
                       with_radii ? (long long*)branch_radii : (long long*)nullptr);
    if (B) hipLaunchKernelGGL(sg_measure_finish_kernel, dim3(sg_blocks(B)), dim3(256), 0, st, (long long*)branches, (long long)B);
    return ru3d_check_launch("skeleton_graph_measure");
}

extern "C" int ru3d_skeleton_graph_erase(uint64_t* skel, int X, int Y, int Z, const int32_t* ids, int64_t n, int64_t M, int64_t B,
                                         const uint8_t* flags_branch, const uint8_t* flags_node, void* ws, size_t ws_bytes,
                                         void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    BV_REQUIRE_SHAPE("skeleton_graph_erase");
    RU3D_REQUIRE(n >= 0 && M >= 0 && B >= 0 && M <= n && B <= n && n <= (int64_t)X * Y * Z,
                 "skeleton_graph_erase: %lld voxels, %lld nodes, %lld branches in %lld voxels of volume", (long long)n,
                 (long long)M, (long long)B, (long long)X * Y * Z);
    RU3D_REQUIRE(skel && ws && (ids || !n) && (flags_node || !M) && (flags_branch || !B),
                 "skeleton_graph_erase: bad argument (null pointer)");
    SG_REQUIRE_WORKSPACE("skeleton_graph_erase");
    if (!n) return 0;
    hipStream_t st = as_stream(stream);
    const sg_geom g = sg_geometry(X, Y, Z);
    const sg_scratch s = sg_carve(ws, g);
    sg_prepare((const sg_u64*)skel, g, s, s.total, nullptr, -1, st);
    hipLaunchKernelGGL(sg_erase_kernel, dim3(sg_blocks(g.words)), dim3(256), 0, st, (sg_u64*)skel, (const int*)s.prefix, g,
                       (const int*)ids, (long long)n, (long long)M, (long long)B, flags_branch, flags_node);
    return ru3d_check_launch("skeleton_graph_erase");
}
