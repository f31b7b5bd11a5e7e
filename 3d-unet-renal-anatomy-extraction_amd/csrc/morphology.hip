// Binary morphology on bit-packed masks and the confusion table of two label volumes (reference nb_post.py:88-112,
// nb.py:11-37): the clean-up and the evaluation of a prediction that stays in HBM.
//
// The packed layout (64 voxels of the contiguous Z axis per 64-bit word) and its geometry helpers are bitvol.h's.
// Invariant of every packed volume written here: the bits at z >= Z of a row's last word are 0.
//   mm_pack_kernel      uint8 volume -> bits under a predicate (== k, or > k which also serves != 0 and >= k).  A lane
//                       compares 16 voxels (one 16-byte load when the rows allow it), four lanes make a word.
//   mm_unpack_kernel    bits -> uint8 volume: write (bit ? value : 0) or paint (bit ? value : what was there).
//   mm_morph_kernel     one erosion or dilation.  The structuring element arrives in the kernel arguments as a list of
//                       (dx, dy, 15-bit mask of z offsets) rows, already reflected for a dilation, so the kernel is a
//                       pure gather: out[p] = AND / OR over the offsets o of in[p + o].  A workgroup owns 8 x 32 rows by
//                       2 words, stages them in LDS with a halo of max|dx|, max|dy| rows and one word on each z side
//                       (outside the volume, and the tail bits: border_value), and every lane produces the two words of
//                       its row: per structure row four LDS reads and per z offset a 64-bit funnel shift and an AND / OR
//                       (two v_alignbit_b32) for each word.  The walk over the structure is wave-uniform (scalar loads of
//                       the arguments, scalar branches on the mask bits, immediate shift counts).  The 32 lanes of a half wave walk y,
//                       and the LDS row pitch is 5 words (odd), so their 8-byte reads fall on 32 distinct bank pairs.
//   mm_confusion_kernel table[min(label, C)][min(pred, C)] += 1 over two uint8 volumes: 16-byte loads, runs of equal
//                       (label, pred) pairs counted in registers, one int32 table per wave in LDS, flushed with 64-bit
//                       integer atomics.  No float anywhere: exact and the same in every run.
#include "common.h"
#include "bitvol.h"

typedef unsigned long long mm_u64;

#define MM_TX 8                           // rows of a morphology tile along x: 8 x 32 rows, one per lane of the workgroup
#define MM_TY 32                          // rows along y: the 32 lanes that share an LDS cycle
#define MM_TW 2                           // output words per lane
#define MM_SW (MM_TW + 2)                 // staged words per row: one halo word on each side
#define MM_PITCH (MM_SW + 1)              // LDS row pitch in words, odd
#define MM_REACH (RU3D_MORPH_MAX_EXTENT / 2)
#define MM_CMAX 32                        // confusion table: classes 0 .. C - 1 and "C or more", C <= 32
#define MM_CTAB ((MM_CMAX + 1) * (MM_CMAX + 1))

// the structure rows as they travel in the kernel arguments: dx | dy << 8 | zmask << 16 in one dword each, because the
// scalar unit loads dwords (a 16-bit field would come through the vector memory path and make the walk divergent)
struct mm_structure {
    int n;
    uint32_t row[RU3D_MORPH_MAX_ROWS];
};

// ------------------------------------------------------------------------------------------------ pack / unpack
__device__ __forceinline__ unsigned mm_test(unsigned v, int eq, int k) { return eq ? (v == (unsigned)k) : ((int)v > k); }

// chunk i = 16 voxels: chunks 4 w .. 4 w + 3 of a row make its word w (the last chunks of a row may lie beyond Z)
template <bool VEC>
__global__ __launch_bounds__(256) void mm_pack_kernel(const uint8_t* __restrict__ src, int Z, int W, int64_t chunks, int eq,
                                                      int k, mm_u64* __restrict__ bits) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    unsigned m = 0;
    if (i < chunks) {
        const int64_t word = i >> 2;
        const int64_t row = word / W;
        const int z0 = (int)(word - row * W) * 64 + (int)(i & 3) * 16;
        const uint8_t* p = src + row * Z + z0;
        if (VEC) {                                      // Z % 16 == 0: a chunk that starts inside the row ends inside it
            if (z0 < Z) {
                const uint4 v = *reinterpret_cast<const uint4*>(p);
                const unsigned q[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int b = 0; b < 16; b++) m |= mm_test((q[b >> 2] >> (8 * (b & 3))) & 0xffu, eq, k) << b;
            }
        } else {
#pragma unroll
            for (int b = 0; b < 16; b++)
                if (z0 + b < Z) m |= mm_test(p[b], eq, k) << b;
        }
    }
    mm_u64 v = (mm_u64)m << (16 * (threadIdx.x & 3));
    v |= __shfl_xor(v, 1, 64);
    v |= __shfl_xor(v, 2, 64);
    if (i < chunks && (threadIdx.x & 3) == 0) bits[i >> 2] = v;
}

template <bool VEC, bool PAINT>
__global__ __launch_bounds__(256) void mm_unpack_kernel(const mm_u64* __restrict__ bits, int Z, int W, int64_t chunks,
                                                        unsigned value, uint8_t* __restrict__ dst) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= chunks) return;
    const int64_t word = i >> 2;
    const int64_t row = word / W;
    const int z0 = (int)(word - row * W) * 64 + (int)(i & 3) * 16;
    if (z0 >= Z) return;
    const unsigned m = (unsigned)(bits[word] >> (16 * (int)(i & 3))) & 0xffffu;
    uint8_t* p = dst + row * Z + z0;
    if (VEC) {
        uint4 o = {0u, 0u, 0u, 0u};
        if (PAINT) {
            if (!m) return;
            o = *reinterpret_cast<const uint4*>(p);
        }
        unsigned q[4] = {o.x, o.y, o.z, o.w};
#pragma unroll
        for (int b = 0; b < 16; b++)
            if (m & (1u << b)) q[b >> 2] = (q[b >> 2] & ~(0xffu << (8 * (b & 3)))) | (value << (8 * (b & 3)));
        *reinterpret_cast<uint4*>(p) = make_uint4(q[0], q[1], q[2], q[3]);
    } else {
#pragma unroll
        for (int b = 0; b < 16; b++) {
            if (z0 + b < Z) {
                if (m & (1u << b))
                    p[b] = (uint8_t)value;
                else if (!PAINT)
                    p[b] = 0;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ erosion / dilation
// bit b of the result = bit b + D of the row whose words around this one are prev, cur, next
// (|D| <= 7).  Written as two 32-bit funnel shifts (v_alignbit_b32, full rate) in place of two 64-bit shifts and an OR.
__device__ __forceinline__ mm_u64 mm_join(unsigned lo, unsigned hi) { return (mm_u64)hi << 32 | lo; }
template <int D>
__device__ __forceinline__ mm_u64 mm_funnel(mm_u64 prev, mm_u64 cur, mm_u64 next) {
    const unsigned clo = (unsigned)cur, chi = (unsigned)(cur >> 32);
    if (D == 0) return cur;
    if (D > 0)          // (cur >> D) | (next << (64 - D))
        return mm_join(__builtin_amdgcn_alignbit(chi, clo, D), __builtin_amdgcn_alignbit((unsigned)next, chi, D));
    // (cur << -D) | (prev >> (64 + D))
    return mm_join(__builtin_amdgcn_alignbit(clo, (unsigned)(prev >> 32), 32 + D), __builtin_amdgcn_alignbit(chi, clo, 32 + D));
}

template <bool DILATE, int K>
__device__ __forceinline__ void mm_combine(unsigned zmask, const mm_u64 (&w)[MM_SW], mm_u64 (&acc)[MM_TW]) {
    if (zmask & (1u << K)) {                               // wave-uniform
#pragma unroll
        for (int j = 0; j < MM_TW; j++) {
            const mm_u64 v = mm_funnel<K - MM_REACH>(w[j], w[j + 1], w[j + 2]);
            acc[j] = DILATE ? (acc[j] | v) : (acc[j] & v);
        }
    }
}

template <bool DILATE>
__global__ __launch_bounds__(256) void mm_morph_kernel(const mm_u64* __restrict__ src, mm_u64* __restrict__ dst, int X, int Y,
                                                       int Z, int W, int rx, int ry, int YT, int WT, mm_u64 border,
                                                       const mm_structure st) {
    extern __shared__ mm_u64 mm_tile[];                    // [MM_TX + 2 rx][MM_TY + 2 ry][MM_PITCH]
    const int PX = MM_TX + 2 * rx, PY = MM_TY + 2 * ry;
    int t = blockIdx.x;
    const int w0 = (t % WT) * MM_TW;
    t /= WT;
    const int y0 = (t % YT) * MM_TY, x0 = (t / YT) * MM_TX;
    const mm_u64 tail = bv_tail(Z);

    const int staged = PX * PY * MM_SW;
    for (int i = threadIdx.x; i < staged; i += 256) {
        const int k = i % MM_SW, r = i / MM_SW;
        const int hx = r / PY, hy = r - hx * PY;
        const int gx = x0 - rx + hx, gy = y0 - ry + hy, gw = w0 - 1 + k;
        mm_u64 v = border;
        if (gx >= 0 && gx < X && gy >= 0 && gy < Y && gw >= 0 && gw < W) {
            v = src[((int64_t)gx * Y + gy) * W + gw];
            if (gw == W - 1) v = (v & ~tail) | (border & tail);
        }
        mm_tile[r * MM_PITCH + k] = v;
    }
    __syncthreads();

    const int lx = threadIdx.x >> 5, ly = threadIdx.x & 31;
    mm_u64 acc[MM_TW];
#pragma unroll
    for (int j = 0; j < MM_TW; j++) acc[j] = DILATE ? 0ull : ~0ull;
    for (int s = 0; s < st.n; s++) {
        const uint32_t row = st.row[s];
        const int dx = (int8_t)(row & 0xffu), dy = (int8_t)((row >> 8) & 0xffu);
        const unsigned zmask = row >> 16;
        const mm_u64* p = mm_tile + ((lx + rx + dx) * PY + (ly + ry + dy)) * MM_PITCH;
        mm_u64 w[MM_SW];
#pragma unroll
        for (int k = 0; k < MM_SW; k++) w[k] = p[k];
        mm_combine<DILATE, 0>(zmask, w, acc);
        mm_combine<DILATE, 1>(zmask, w, acc);
        mm_combine<DILATE, 2>(zmask, w, acc);
        mm_combine<DILATE, 3>(zmask, w, acc);
        mm_combine<DILATE, 4>(zmask, w, acc);
        mm_combine<DILATE, 5>(zmask, w, acc);
        mm_combine<DILATE, 6>(zmask, w, acc);
        mm_combine<DILATE, 7>(zmask, w, acc);
        mm_combine<DILATE, 8>(zmask, w, acc);
        mm_combine<DILATE, 9>(zmask, w, acc);
        mm_combine<DILATE, 10>(zmask, w, acc);
        mm_combine<DILATE, 11>(zmask, w, acc);
        mm_combine<DILATE, 12>(zmask, w, acc);
        mm_combine<DILATE, 13>(zmask, w, acc);
        mm_combine<DILATE, 14>(zmask, w, acc);
    }

    const int x = x0 + lx, y = y0 + ly;
    if (x < X && y < Y) {
#pragma unroll
        for (int j = 0; j < MM_TW; j++) {
            const int gw = w0 + j;
            if (gw < W) dst[((int64_t)x * Y + y) * W + gw] = gw == W - 1 ? acc[j] & ~tail : acc[j];
        }
    }
}

// ------------------------------------------------------------------------------------------------ confusion table
__global__ __launch_bounds__(256) void mm_zero_table_kernel(long long* __restrict__ table, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) table[i] = 0;
}

struct mm_run {
    int key, count;
};
__device__ __forceinline__ void mm_count(mm_run& run, int* tab, unsigned label, unsigned pred, int C) {
    const int key = (int)min(label, (unsigned)C) * (C + 1) + (int)min(pred, (unsigned)C);
    if (key == run.key) {
        run.count++;
    } else {
        if (run.count) atomicAdd(&tab[run.key], run.count);
        run.key = key;
        run.count = 1;
    }
}

// Elements [0, head) and [head + 16 vecs, n) are read a byte at a time, the `vecs` 16-byte pieces in between with one load
// per operand (the host puts `head` where both pointers reach a 16-byte boundary, or makes everything head).
__global__ __launch_bounds__(256) void mm_confusion_kernel(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ label,
                                                           int64_t n, int64_t head, int64_t vecs, int C,
                                                           unsigned long long* __restrict__ table) {
    __shared__ int tabs[4][MM_CTAB];
    const int K = C + 1;
    for (int i = threadIdx.x; i < 4 * MM_CTAB; i += 256) (&tabs[0][0])[i] = 0;
    __syncthreads();
    int* tab = tabs[threadIdx.x >> 6];
    mm_run run = {0, 0};
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
    for (int64_t i = tid; i < vecs; i += stride) {
        const uint4 pv = *reinterpret_cast<const uint4*>(pred + head + 16 * i);
        const uint4 lv = *reinterpret_cast<const uint4*>(label + head + 16 * i);
        const unsigned pq[4] = {pv.x, pv.y, pv.z, pv.w}, lq[4] = {lv.x, lv.y, lv.z, lv.w};
#pragma unroll
        for (int b = 0; b < 16; b++)
            mm_count(run, tab, (lq[b >> 2] >> (8 * (b & 3))) & 0xffu, (pq[b >> 2] >> (8 * (b & 3))) & 0xffu, C);
    }
    const int64_t body_end = head + 16 * vecs, loose = head + (n - body_end);
    for (int64_t i = tid; i < loose; i += stride) {
        const int64_t e = i < head ? i : body_end + (i - head);
        mm_count(run, tab, label[e], pred[e], C);
    }
    if (run.count) atomicAdd(&tab[run.key], run.count);
    __syncthreads();
    for (int i = threadIdx.x; i < K * K; i += 256) {
        const long long s = (long long)tabs[0][i] + tabs[1][i] + tabs[2][i] + tabs[3][i];
        if (s) atomicAdd(&table[i], (unsigned long long)s);
    }
}

// ------------------------------------------------------------------------------------------------ host side
static inline bool mm_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

extern "C" size_t ru3d_mask_bytes(int X, int Y, int Z) {
    if (!bv_shape_ok(X, Y, Z)) return 0;
    return (size_t)X * Y * bv_words(Z) * sizeof(mm_u64);
}

extern "C" int ru3d_mask_pack(const uint8_t* src, int X, int Y, int Z, int op, int value, uint64_t* bits, void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    BV_REQUIRE_SHAPE("mask_pack");
    RU3D_REQUIRE(src && bits, "mask_pack: bad argument (null pointer)");
    RU3D_REQUIRE(op >= RU3D_MASK_NE && op <= RU3D_MASK_GE, "mask_pack: predicate %d (RU3D_MASK_NE .. RU3D_MASK_GE)", op);
    RU3D_REQUIRE(value >= 0 && value <= 255, "mask_pack: value %d is not a uint8", value);
    const int eq = op == RU3D_MASK_EQ;
    const int k = op == RU3D_MASK_NE ? 0 : (op == RU3D_MASK_GE ? value - 1 : value);        // v >= k  <=>  v > k - 1
    const int W = bv_words(Z);
    const int64_t chunks = (int64_t)X * Y * W * 4;
    const unsigned blocks = (unsigned)((chunks + 255) / 256);
    hipStream_t st = as_stream(stream);
    if (Z % 16 == 0 && mm_aligned16(src))
        hipLaunchKernelGGL(mm_pack_kernel<true>, dim3(blocks), dim3(256), 0, st, src, Z, W, chunks, eq, k, (mm_u64*)bits);
    else
        hipLaunchKernelGGL(mm_pack_kernel<false>, dim3(blocks), dim3(256), 0, st, src, Z, W, chunks, eq, k, (mm_u64*)bits);
    return ru3d_check_launch("mask_pack");
}

extern "C" int ru3d_mask_unpack(const uint64_t* bits, int X, int Y, int Z, int value, int paint, uint8_t* dst,
                                void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    BV_REQUIRE_SHAPE("mask_unpack");
    RU3D_REQUIRE(bits && dst, "mask_unpack: bad argument (null pointer)");
    RU3D_REQUIRE(value >= 0 && value <= 255, "mask_unpack: value %d is not a uint8", value);
    RU3D_REQUIRE(paint == 0 || paint == 1, "mask_unpack: paint %d (0 = write, 1 = paint)", paint);
    const int W = bv_words(Z);
    const int64_t chunks = (int64_t)X * Y * W * 4;
    const dim3 grid((unsigned)((chunks + 255) / 256)), block(256);
    hipStream_t st = as_stream(stream);
    const mm_u64* b = (const mm_u64*)bits;
    const unsigned v = (unsigned)value;
    if (Z % 16 == 0 && mm_aligned16(dst)) {
        if (paint)
            hipLaunchKernelGGL((mm_unpack_kernel<true, true>), grid, block, 0, st, b, Z, W, chunks, v, dst);
        else
            hipLaunchKernelGGL((mm_unpack_kernel<true, false>), grid, block, 0, st, b, Z, W, chunks, v, dst);
    } else {
        if (paint)
            hipLaunchKernelGGL((mm_unpack_kernel<false, true>), grid, block, 0, st, b, Z, W, chunks, v, dst);
        else
            hipLaunchKernelGGL((mm_unpack_kernel<false, false>), grid, block, 0, st, b, Z, W, chunks, v, dst);
    }
    return ru3d_check_launch("mask_unpack");
}

extern "C" int ru3d_binary_morph(const uint64_t* src, uint64_t* dst, int X, int Y, int Z, int op, const ru3d_morph_row* rows,
                                 int num_rows, int border_value, void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    BV_REQUIRE_SHAPE("binary_morph");
    RU3D_REQUIRE(src && dst && rows, "binary_morph: bad argument (null pointer)");
    RU3D_REQUIRE(src != dst, "binary_morph: not an in-place operation (src == dst)");
    RU3D_REQUIRE(op == RU3D_MORPH_ERODE || op == RU3D_MORPH_DILATE, "binary_morph: op %d (RU3D_MORPH_ERODE / _DILATE)", op);
    RU3D_REQUIRE(border_value == 0 || border_value == 1, "binary_morph: border_value %d (0 or 1)", border_value);
    RU3D_REQUIRE(num_rows >= 1 && num_rows <= RU3D_MORPH_MAX_ROWS, "binary_morph: %d structure rows (1 .. %d)", num_rows,
                 RU3D_MORPH_MAX_ROWS);
    mm_structure st;
    st.n = num_rows;
    int rx = 0, ry = 0;
    for (int i = 0; i < num_rows; i++) {
        const int dx = rows[i].dx, dy = rows[i].dy;
        RU3D_REQUIRE(dx >= -MM_REACH && dx <= MM_REACH && dy >= -MM_REACH && dy <= MM_REACH,
                     "binary_morph: structure row %d at (%d, %d): extents above %d", i, dx, dy, RU3D_MORPH_MAX_EXTENT);
        RU3D_REQUIRE(rows[i].zmask != 0 && rows[i].zmask < (1u << RU3D_MORPH_MAX_EXTENT),
                     "binary_morph: structure row %d has the z mask 0x%x (1 .. 0x7fff)", i, (unsigned)rows[i].zmask);
        st.row[i] = (uint32_t)(uint8_t)rows[i].dx | (uint32_t)(uint8_t)rows[i].dy << 8 | (uint32_t)rows[i].zmask << 16;
        rx = abs(dx) > rx ? abs(dx) : rx;
        ry = abs(dy) > ry ? abs(dy) : ry;
    }
    for (int i = num_rows; i < RU3D_MORPH_MAX_ROWS; i++) st.row[i] = 0;
    const int W = bv_words(Z);
    const int XT = (X + MM_TX - 1) / MM_TX, YT = (Y + MM_TY - 1) / MM_TY, WT = (W + MM_TW - 1) / MM_TW;
    const int64_t tiles = (int64_t)XT * YT * WT;
    RU3D_REQUIRE(tiles < ((int64_t)1 << 31), "binary_morph: %lld tiles", (long long)tiles);
    const size_t lds = (size_t)(MM_TX + 2 * rx) * (MM_TY + 2 * ry) * MM_PITCH * sizeof(mm_u64);    // <= 40,480 bytes
    const mm_u64 border = border_value ? ~0ull : 0ull;
    hipStream_t hs = as_stream(stream);
    if (op == RU3D_MORPH_DILATE)
        hipLaunchKernelGGL(mm_morph_kernel<true>, dim3((unsigned)tiles), dim3(256), lds, hs, (const mm_u64*)src, (mm_u64*)dst,
                           X, Y, Z, W, rx, ry, YT, WT, border, st);
    else
        hipLaunchKernelGGL(mm_morph_kernel<false>, dim3((unsigned)tiles), dim3(256), lds, hs, (const mm_u64*)src, (mm_u64*)dst,
                           X, Y, Z, W, rx, ry, YT, WT, border, st);
    return ru3d_check_launch("binary_morph");
}

extern "C" int ru3d_confusion_counts(const uint8_t* pred, const uint8_t* label, int64_t n, int num_classes, int64_t* table,
                                     void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    RU3D_REQUIRE(pred && label && table, "confusion_counts: bad argument (null pointer)");
    RU3D_REQUIRE(num_classes >= 1 && num_classes <= MM_CMAX, "confusion_counts: %d classes (1 .. %d)", num_classes, MM_CMAX);
    RU3D_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "confusion_counts: %lld voxels (0 .. 2^31 - 1)", (long long)n);
    hipStream_t st = as_stream(stream);
    const int cells = (num_classes + 1) * (num_classes + 1);
    hipLaunchKernelGGL(mm_zero_table_kernel, dim3((cells + 255) / 256), dim3(256), 0, st, (long long*)table, cells);
    if (n > 0) {
        int64_t head = n, vecs = 0;                        // operands that reach a 16-byte boundary together: vector body
        if ((((uintptr_t)pred ^ (uintptr_t)label) & 15) == 0) {
            head = (int64_t)((16 - ((uintptr_t)pred & 15)) & 15);
            head = head < n ? head : n;
            vecs = (n - head) / 16;
        }
        const int64_t work = vecs + (n - 16 * vecs);       // loop trips summed over the grid
        int64_t blocks = (work + 255) / 256;
        const int64_t cap = (int64_t)ru3d_get_cu_budget() * 8;
        blocks = blocks > cap ? cap : blocks;
        hipLaunchKernelGGL(mm_confusion_kernel, dim3((unsigned)(blocks < 1 ? 1 : blocks)), dim3(256), 0, st, pred, label, n,
                           head, vecs, num_classes, (unsigned long long*)table);
    }
    return ru3d_check_launch("confusion_counts");
}
