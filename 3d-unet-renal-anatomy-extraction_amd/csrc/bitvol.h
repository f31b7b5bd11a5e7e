// Bit-packed volumes and stream compaction: the one definition of what components, morphology, prepare, distance, mesh,
// render, skeleton and boundary share.
//
// A packed mask holds 64 voxels of the contiguous Z axis in one 64-bit word: bit b of word w of row (x, y) is voxel
// z = 64 w + b, a row has W = bv_words(Z) words, rows follow each other in the volume's [X, Y] order, and the bits at
// z >= Z of a row's last word (bv_tail) are 0 in every packed volume the library writes.
//
// Compaction (the elements of a list that pass a test, written in element order without an atomic) is three launches:
// a count per chunk (bv_chunk_sum), one workgroup that turns the chunk counts into exclusive prefix sums
// (bv_scan_chunks), and a pass in which every lane adds its rank inside the chunk (bv_chunk_rank for a count per lane,
// bv_ballot_rank for a flag per lane) to its chunk's offset.  The pieces are device functions; the kernels, their
// grids and their epilogues belong to the callers.  Chunk workgroups have BV_CHUNK_THREADS threads, the scan
// BV_SCAN_THREADS.
//
// Nothing here does floating-point arithmetic: bv_block_join moves the values and applies the caller's functor in a
// fixed order, so a caller compiled with contraction off keeps its bits.
#pragma once
#include "common.h"

typedef unsigned long long bv_u64;

#define BV_CHUNK_THREADS 256
#define BV_CHUNK_WAVES (BV_CHUNK_THREADS / RU3D_WAVE)
#define BV_SCAN_THREADS 1024

// ------------------------------------------------------------------------------------------------ geometry
// words of a packed row of Z voxels
__host__ __device__ static inline int bv_words(int Z) { return (Z + 63) / 64; }
// the bits at z >= Z of a row's last word
__host__ __device__ static inline bv_u64 bv_tail(int Z) { return (Z & 63) ? (~0ull << (Z & 63)) : 0ull; }
// workspace sections start on 256-byte boundaries
static inline size_t bv_align(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
// every extent positive and fewer than 2^31 voxels: a linear voxel index is an int
static inline bool bv_shape_ok(int X, int Y, int Z) {
    return X > 0 && Y > 0 && Z > 0 && (int64_t)X * Y * Z < ((int64_t)1 << 31);
}
// log2 of the columns of z that an LDS tile of a scanned axis of L voxels holds: the largest power of two T with
// L * T <= tile_elems, at most max_cols and no more than Z needs
static inline int bv_tile_shift(int L, int Z, int max_cols, int tile_elems) {
    int s = 0;
    while ((2 << s) <= max_cols && (int64_t)L * (2 << s) <= tile_elems && (1 << s) < Z) s++;
    return s;
}

#define BV_REQUIRE_SHAPE(what)                                                                                       \
    RU3D_REQUIRE(bv_shape_ok(X, Y, Z), what ": a %dx%dx%d volume is not supported (every extent positive, X*Y*Z < 2^31)", \
                 X, Y, Z)

// ------------------------------------------------------------------------------------------------ word access
// word w of row (x, y) of a packed [X][Y][W] volume as it is stored; 0 outside the volume
__device__ __forceinline__ bv_u64 bv_word(const bv_u64* __restrict__ bits, int X, int Y, int W, int x, int y, int w) {
    if ((unsigned)x >= (unsigned)X || (unsigned)y >= (unsigned)Y || (unsigned)w >= (unsigned)W) return 0ull;
    return bits[((int64_t)x * Y + y) * W + w];
}
// the same for an input that may carry set bits at z >= Z: `tail` (bv_tail) is cleared from a row's last word
__device__ __forceinline__ bv_u64 bv_word_masked(const bv_u64* __restrict__ bits, int X, int Y, int W, bv_u64 tail, int x,
                                                 int y, int w) {
    if ((unsigned)x >= (unsigned)X || (unsigned)y >= (unsigned)Y || (unsigned)w >= (unsigned)W) return 0ull;
    const bv_u64 v = bits[((int64_t)x * Y + y) * W + w];
    return w == W - 1 ? v & ~tail : v;
}
// a row seen from one voxel further along z, from its words w - 1, w, w + 1 = prev, cur, next:
// bit b of bv_zdown is voxel z - 1, bit b of bv_zup voxel z + 1 (z = 64 w + b); a missing word is 0
__device__ __forceinline__ bv_u64 bv_zdown(bv_u64 prev, bv_u64 cur) { return cur << 1 | prev >> 63; }
__device__ __forceinline__ bv_u64 bv_zup(bv_u64 cur, bv_u64 next) { return cur >> 1 | next << 63; }
// bit b = voxel z + dz, dz in -1, 0, 1
__device__ __forceinline__ bv_u64 bv_zview(bv_u64 prev, bv_u64 cur, bv_u64 next, int dz) {
    return dz == 0 ? cur : (dz > 0 ? bv_zup(cur, next) : bv_zdown(prev, cur));
}

// distance in voxels from z to the nearest set bit of (row ^ inv), -1 when there is none.  row: the W words of a packed
// row; last: the bits at z < Z of its last word (~bv_tail); inv: 0 to look for a set bit, ~0 for a clear one.
__device__ __forceinline__ int bv_nearest(const bv_u64* __restrict__ row, int W, bv_u64 last, bv_u64 inv, int z) {
    const int w = z >> 6, b = z & 63;
    const bv_u64 cur = (row[w] ^ inv) & (w == W - 1 ? last : ~0ull);
    int best = -1;
    bv_u64 m = cur & (~0ull >> (63 - b));                                   // the bits at or below z
    if (m) {
        best = b - (63 - __clzll(m));
    } else {
        for (int k = w - 1; k >= 0; k--) {
            const bv_u64 v = row[k] ^ inv;
            if (v) {
                best = z - (64 * k + 63 - __clzll(v));
                break;
            }
        }
    }
    m = cur & (~0ull << b);                                                 // the bits at or above z
    int up = -1;
    if (m) {
        up = __ffsll(m) - 1 - b;
    } else {
        for (int k = w + 1; k < W; k++) {
            const bv_u64 v = (row[k] ^ inv) & (k == W - 1 ? last : ~0ull);
            if (v) {
                up = 64 * k + __ffsll(v) - 1 - z;
                break;
            }
        }
    }
    if (up >= 0 && (best < 0 || up < best)) best = up;
    return best;
}

// ------------------------------------------------------------------------------------------------ compaction
__device__ __forceinline__ int bv_wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// counts[blockIdx.x] = the sum of c over the BV_CHUNK_THREADS lanes of the workgroup.  Every lane calls it, once.
__device__ __forceinline__ void bv_chunk_sum(int c, int* __restrict__ counts) {
    __shared__ int s_part[BV_CHUNK_WAVES];
    c = bv_wave_sum(c);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = s_part[0] + s_part[1] + s_part[2] + s_part[3];
}

// counts[0 .. chunks) -> their exclusive prefix sums in place, summed in S and stored as int (meaningless once a sum
// reaches 2^31, which an S of 64 bits tells); returns the grand total to every thread.  One workgroup of
// BV_SCAN_THREADS threads, thread t owns ceil(chunks / BV_SCAN_THREADS) consecutive counts; s_sum: BV_SCAN_THREADS
// elements of LDS.
template <typename S>
__device__ __forceinline__ S bv_scan_chunks(int* __restrict__ counts, int chunks, S* s_sum) {
    const int per = (chunks + BV_SCAN_THREADS - 1) / BV_SCAN_THREADS;
    const int lo = min(chunks, (int)threadIdx.x * per), hi = min(chunks, lo + per);
    S sum = 0;
    for (int i = lo; i < hi; i++) sum += counts[i];
    s_sum[threadIdx.x] = sum;
    __syncthreads();
    for (int off = 1; off < BV_SCAN_THREADS; off <<= 1) {                   // inclusive Hillis-Steele over the per-thread sums
        const S v = (int)threadIdx.x >= off ? s_sum[threadIdx.x - off] : 0;
        __syncthreads();
        s_sum[threadIdx.x] += v;
        __syncthreads();
    }
    S run = s_sum[threadIdx.x] - sum;
    for (int i = lo; i < hi; i++) {
        const int c = counts[i];
        counts[i] = (int)run;
        run += c;
    }
    return s_sum[BV_SCAN_THREADS - 1];
}

// the sum of c over the lanes of the workgroup (BV_CHUNK_THREADS) in front of this one: an inclusive scan by shuffles
// inside the wave, then the waves before it.  Every lane calls it, once.
__device__ __forceinline__ int bv_chunk_rank(int c) {
    __shared__ int s_part[BV_CHUNK_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(incl, o, 64);
        if (lane >= o) incl += v;
    }
    if (lane == 63) s_part[wave] = incl;
    __syncthreads();
    int rank = incl - c;
    for (int k = 0; k < wave; k++) rank += s_part[k];
    return rank;
}

// the number of flagged lanes of the workgroup (BV_CHUNK_THREADS) in front of this one, *all = the flagged lanes of the
// whole workgroup.  s_part: BV_CHUNK_WAVES ints of LDS, read after the one barrier in here: a caller that comes back
// with the same s_part puts a barrier in between, or alternates between two.
__device__ __forceinline__ int bv_ballot_rank(bool flag, int* s_part, int* all) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bv_u64 m = __ballot(flag);
    if (lane == 0) s_part[wave] = __popcll(m);
    __syncthreads();
    int before = 0, sum = 0;
#pragma unroll
    for (int w = 0; w < BV_CHUNK_WAVES; w++) {
        const int c = s_part[w];
        before += w < wave ? c : 0;
        sum += c;
    }
    *all = sum;
    return before + __popcll(m & (((bv_u64)1 << lane) - 1));
}

// the value of lane (lane ^ o) of the wave, for any plain struct of 32-bit multiples
template <typename T>
__device__ __forceinline__ T bv_shfl_xor(const T& v, int o) {
    static_assert(sizeof(T) % sizeof(int) == 0, "bv_shfl_xor moves 32-bit pieces");
    int p[sizeof(T) / sizeof(int)];
    __builtin_memcpy(p, &v, sizeof(T));
#pragma unroll
    for (size_t k = 0; k < sizeof(T) / sizeof(int); k++) p[k] = __shfl_xor(p[k], o, 64);
    T r;
    __builtin_memcpy(&r, p, sizeof(T));
    return r;
}

// the join of v over the workgroup (BV_CHUNK_THREADS) in thread 0, in a fixed order whatever the values: a butterfly
// inside each wave (partner 32, 16, .. 1, own value on the left), then (wave 0 + wave 1) + (wave 2 + wave 3).
// s_part: BV_CHUNK_WAVES elements of LDS, free for the next call on return.
template <typename T, typename J>
__device__ __forceinline__ T bv_block_join(T v, T* s_part, J join) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = join(v, bv_shfl_xor(v, o));
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) v = join(join(s_part[0], s_part[1]), join(s_part[2], s_part[3]));
    __syncthreads();
    return v;
}
