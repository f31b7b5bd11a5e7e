// Dataset preparation on the device (reference data.py:117-172 orient_crop_case, 322-461 analyze_cases /
// analyze_raw_cases): the three things the preparation of a case needs that are not plain data movement.
//   pp_bbox_kernel         the box of the voxels with any channel above a threshold, and their number.  One streaming
//                          pass over the fp32 [X, Y, Z, C] case: a lane takes four voxels (C 16-byte loads) and keeps
//                          running minima / maxima of their indices; wave reduction, LDS across the four waves, then one
//                          integer atomicMin / atomicMax per workgroup and bound.  Integer atomics: the same bits whatever
//                          the arrival order.
//   pp_fg_count / pp_scan / pp_sample_scatter
//                          image[..., c][label > 0][::stride] in numpy's element order: bitvol.h's compaction over
//                          2048-voxel chunks.  A voxel's rank among the foreground is its chunk's offset + the eight
//                          ballot ranks of the chunk so far, and rank r goes to slot r / stride when r % stride == 0.
//                          No atomic decides an output position.
//   pp_hist / pp_select    exact order statistics by radix select on the order-preserving 32-bit key of a float, eight
//                          bits per pass, most significant first.  Every rank carries its own prefix; a pass counts, per
//                          rank, the next digit of the values that match the prefix (LDS histogram, integer atomics, one
//                          global add per non-empty bin and workgroup), and one workgroup picks each rank's bin.  Nothing
//                          is sorted or moved; the values are read once per pass.
//   pp_moments_*           n, min, max, mean and the population standard deviation in float64: two passes (sum, then
//                          squared deviations from the mean), per-workgroup partials in a slab, summed by one workgroup
//                          in a fixed order.  No float atomics: two runs give the same bits.
#include "common.h"
#include "bitvol.h"
#include "select_key.h"
#include <limits.h>

#define PP_WAVES (PP_THREADS / RU3D_WAVE)
#define PP_CHUNK 2048                        // voxels per workgroup of the masked sample
#define PP_BINS 256                          // radix select: 8 bits per pass
#define PP_PASSES 4
#define PP_MAX_RANKS RU3D_ORDER_STATS_MAX_RANKS
#define PP_MAX_BLOCKS 2048                   // slab rows of the moments; also the cap of every streaming grid here

typedef unsigned long long pp_u64;

static inline bool pp_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
// grid of a grid-stride pass over `items` work items, one per thread and trip
static unsigned pp_stream_blocks(int64_t items) {
    int64_t blocks = (items + PP_THREADS - 1) / PP_THREADS;
    int64_t cap = (int64_t)ru3d_get_cu_budget() * 8;
    cap = cap > PP_MAX_BLOCKS ? PP_MAX_BLOCKS : cap;
    blocks = blocks > cap ? cap : blocks;
    return (unsigned)(blocks < 1 ? 1 : blocks);
}

#define PP_REQUIRE_SHAPE(what)                                                                                       \
    RU3D_REQUIRE(bv_shape_ok(X, Y, Z), what ": volume %d x %d x %d is not supported (every extent >= 1, fewer than 2^31 " \
                                            "voxels)", X, Y, Z)

__device__ __forceinline__ int pp_wave_min(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ int pp_wave_max(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return v;
}

// ------------------------------------------------------------------------------------------------ a. threshold box
struct pp_box {
    int lo[3], hi[3], cnt;
    __device__ __forceinline__ void visit(int x, int y, int z) {
        lo[0] = min(lo[0], x), hi[0] = max(hi[0], x);
        lo[1] = min(lo[1], y), hi[1] = max(hi[1], y);
        lo[2] = min(lo[2], z), hi[2] = max(hi[2], z);
        cnt++;
    }
};

__global__ __launch_bounds__(64) void pp_bbox_init_kernel(int* __restrict__ box, pp_u64* __restrict__ count) {
    if (threadIdx.x < 6) box[threadIdx.x] = (threadIdx.x & 1) ? -1 : INT_MAX;
    if (threadIdx.x == 6) *count = 0;
}

// CT > 0: C == CT and the image is 16-byte aligned - a lane takes voxels 4 q .. 4 q + 3 with CT 16-byte loads, the last
// n % 4 voxels go one per lane.  CT == 0: any C, any alignment, one voxel per lane and trip.
template <int CT>
__global__ __launch_bounds__(PP_THREADS) void pp_bbox_kernel(const float* __restrict__ img, int Y, int Z, int C, int n,
                                                             float thr, int* __restrict__ box, pp_u64* __restrict__ count) {
    __shared__ int s_red[PP_WAVES][7];
    pp_box b = {{INT_MAX, INT_MAX, INT_MAX}, {-1, -1, -1}, 0};
    const int stride = (int)gridDim.x * PP_THREADS;                        // <= 2^19
    const int first = (int)blockIdx.x * PP_THREADS + (int)threadIdx.x;
    int scalar_from = 0;
    if (CT > 0) {
        const int quads = n >> 2;
        scalar_from = quads << 2;
        for (int q = first; q < quads; q += stride) {
            const float4* p = reinterpret_cast<const float4*>(img) + (int64_t)q * CT;
            float v[4 * (CT > 0 ? CT : 1)];
#pragma unroll
            for (int i = 0; i < CT; i++) {
                const float4 t = p[i];
                v[4 * i] = t.x, v[4 * i + 1] = t.y, v[4 * i + 2] = t.z, v[4 * i + 3] = t.w;
            }
            unsigned m = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                bool above = false;
#pragma unroll
                for (int c = 0; c < CT; c++) above |= v[k * CT + c] > thr;
                m |= (unsigned)above << k;
            }
            if (m) {                                                       // air costs no index arithmetic
                const int v0 = q << 2, r = v0 / Z;
                int z = v0 - r * Z, x = r / Y, y = r - x * Y;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    if (m >> k & 1) b.visit(x, y, z);
                    if (++z == Z) {
                        z = 0;
                        if (++y == Y) y = 0, x++;
                    }
                }
            }
        }
    }
    for (int64_t i = (int64_t)scalar_from + first; i < n; i += stride) {
        const float* p = img + i * C;
        bool above = false;
        for (int c = 0; c < C; c++) above |= p[c] > thr;
        if (above) {
            const int r = (int)i / Z, x = r / Y;
            b.visit(x, r - x * Y, (int)i - r * Z);
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int a = 0; a < 3; a++) b.lo[a] = pp_wave_min(b.lo[a]), b.hi[a] = pp_wave_max(b.hi[a]);
    b.cnt = bv_wave_sum(b.cnt);
    if (lane == 0) {
#pragma unroll
        for (int a = 0; a < 3; a++) s_red[wave][2 * a] = b.lo[a], s_red[wave][2 * a + 1] = b.hi[a];
        s_red[wave][6] = b.cnt;
    }
    __syncthreads();
    if (threadIdx.x < 7) {
        const int j = threadIdx.x;
        int v = s_red[0][j];
        for (int w = 1; w < PP_WAVES; w++)
            v = j == 6 ? v + s_red[w][j] : ((j & 1) ? max(v, s_red[w][j]) : min(v, s_red[w][j]));
        const int total = s_red[0][6] + s_red[1][6] + s_red[2][6] + s_red[3][6];
        if (total > 0) {                                                   // one atomic per workgroup and bound
            if (j == 6) atomicAdd(count, (pp_u64)v);
            else if (j & 1) atomicMax(box + j, v);
            else atomicMin(box + j, v);
        }
    }
}

// ------------------------------------------------------------------------------------------------ b. masked sample
template <typename L>
__global__ __launch_bounds__(PP_THREADS) void pp_fg_count_kernel(const L* __restrict__ lab, int n, int* __restrict__ counts) {
    const int64_t base = (int64_t)blockIdx.x * PP_CHUNK;
    int c = 0;
#pragma unroll
    for (int k = 0; k < PP_CHUNK / PP_THREADS; k++) {
        const int64_t i = base + k * PP_THREADS + threadIdx.x;
        if (i < n) c += lab[i] > 0;
    }
    bv_chunk_sum(c, counts);
}

// bv_scan_chunks over the chunk counts; the number of samples ceil(total / stride) -> *samples_out
__global__ __launch_bounds__(BV_SCAN_THREADS) void pp_scan_kernel(int* __restrict__ counts, int chunks, int stride,
                                                                   long long* __restrict__ samples_out) {
    __shared__ int s_sum[BV_SCAN_THREADS];
    const int sum = bv_scan_chunks(counts, chunks, s_sum);
    if (threadIdx.x == BV_SCAN_THREADS - 1) *samples_out = ((long long)sum + stride - 1) / stride;
}

template <typename L>
__global__ __launch_bounds__(PP_THREADS) void pp_sample_scatter_kernel(const float* __restrict__ img, int C, int channel,
                                                                       const L* __restrict__ lab, int n, int stride,
                                                                       const int* __restrict__ offsets,
                                                                       float* __restrict__ out, long long capacity) {
    __shared__ int s_part[2][PP_WAVES];                                    // two sets: one barrier per trip
    const int64_t base = (int64_t)blockIdx.x * PP_CHUNK;
    int run = offsets[blockIdx.x];
#pragma unroll 1
    for (int k = 0; k < PP_CHUNK / PP_THREADS; k++) {
        const int64_t i = base + k * PP_THREADS + threadIdx.x;
        const bool fg = i < n && lab[i] > 0;
        int all;
        const int before = bv_ballot_rank(fg, s_part[k & 1], &all);
        if (fg) {
            const int r = run + before;
            const int slot = r / stride;
            if (r - slot * stride == 0 && slot < capacity) out[slot] = img[i * C + channel];
        }
        run += all;
    }
}

// ------------------------------------------------------------------------------------------------ c. order statistics
// pp_key / pp_unkey and the streaming reader pp_stream: select_key.h
struct pp_select_state {
    unsigned prefix[PP_MAX_RANKS];           // the digits chosen so far, most significant first
    long long k[PP_MAX_RANKS];               // the rank that is left among the values that share the prefix
};
struct pp_ranks {
    long long k[PP_MAX_RANKS];
};

// pass 0 counts the top digit of every value into histogram 0 (no rank has a prefix yet); pass p > 0 counts, for each rank,
// digit p of the values whose digits 0 .. p - 1 equal that rank's prefix.  hist: this pass's [R][256] table, zeroed.
__global__ __launch_bounds__(PP_THREADS) void pp_hist_kernel(const float* __restrict__ v, int64_t n, int pass, int R,
                                                             const pp_select_state* __restrict__ st,
                                                             pp_u64* __restrict__ hist) {
    __shared__ unsigned s_hist[PP_MAX_RANKS * PP_BINS];
    __shared__ unsigned s_prefix[PP_MAX_RANKS];
    const int tables = pass == 0 ? 1 : R;
    for (int i = threadIdx.x; i < tables * PP_BINS; i += PP_THREADS) s_hist[i] = 0;
    if (pass > 0 && (int)threadIdx.x < R) s_prefix[threadIdx.x] = st->prefix[threadIdx.x];
    __syncthreads();
    if (pass == 0) {
        pp_stream(v, n, [&](float x) { atomicAdd(&s_hist[pp_key(x) >> 24], 1u); });
    } else {
        const int shift = 24 - 8 * pass;
        pp_stream(v, n, [&](float x) {
            const unsigned key = pp_key(x), hi = key >> (shift + 8), digit = (key >> shift) & (PP_BINS - 1);
            for (int r = 0; r < R; r++)
                if (hi == s_prefix[r]) atomicAdd(&s_hist[r * PP_BINS + digit], 1u);
        });
    }
    __syncthreads();
    for (int i = threadIdx.x; i < tables * PP_BINS; i += PP_THREADS) {
        const unsigned c = s_hist[i];
        if (c) atomicAdd(hist + i, (pp_u64)c);
    }
}

// One workgroup of 256 threads, thread t = bin t: for each rank the bin whose running count passes the rank that is left.
__global__ __launch_bounds__(PP_BINS) void pp_select_kernel(int pass, int R, pp_ranks first, pp_select_state* __restrict__ st,
                                                            const pp_u64* __restrict__ hist, float* __restrict__ out) {
    __shared__ pp_u64 s_cum[PP_BINS];
    const int t = threadIdx.x;
    for (int r = 0; r < R; r++) {
        const pp_u64 h = hist[(pass == 0 ? 0 : r) * PP_BINS + t];
        const pp_u64 k = (pp_u64)(pass == 0 ? first.k[r] : st->k[r]);      // every lane reads it before the barriers below
        s_cum[t] = h;
        __syncthreads();
        for (int off = 1; off < PP_BINS; off <<= 1) {
            const pp_u64 a = t >= off ? s_cum[t - off] : 0;
            __syncthreads();
            s_cum[t] += a;
            __syncthreads();
        }
        const pp_u64 incl = s_cum[t], excl = incl - h;
        if (h != 0 && k >= excl && k < incl) {                             // exactly one bin: the bins tile [0, count)
            const unsigned prefix = ((pass == 0 ? 0u : st->prefix[r]) << 8) | (unsigned)t;
            st->prefix[r] = prefix;
            st->k[r] = (long long)(k - excl);
            if (pass == PP_PASSES - 1) out[r] = pp_unkey(prefix);
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------ d. moments
// slab[block][3] = (sum, min, max) in pass 0, (sum of squared deviations from out[3], -, -) in pass 1
template <int PASS>
__global__ __launch_bounds__(PP_THREADS) void pp_moments_partial_kernel(const float* __restrict__ v, int64_t n,
                                                                        const double* __restrict__ out,
                                                                        double* __restrict__ slab) {
    __shared__ double s_red[PP_WAVES][3];
    double s = 0.0;
    float lo = INFINITY, hi = -INFINITY;
    if (PASS == 0) {
        pp_stream(v, n, [&](float x) {
            s += (double)x;
            lo = fminf(lo, x), hi = fmaxf(hi, x);
        });
    } else {
        const double mean = out[3];
        pp_stream(v, n, [&](float x) {
            const double d = (double)x - mean;
            s += d * d;
        });
    }
    s = wave_sum_d(s);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) lo = fminf(lo, __shfl_xor(lo, o, 64)), hi = fmaxf(hi, __shfl_xor(hi, o, 64));
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) s_red[wave][0] = s, s_red[wave][1] = (double)lo, s_red[wave][2] = (double)hi;
    __syncthreads();
    if (threadIdx.x == 0) {
        double* row = slab + (int64_t)blockIdx.x * 3;
        row[0] = ((s_red[0][0] + s_red[1][0]) + s_red[2][0]) + s_red[3][0];
        row[1] = fmin(fmin(s_red[0][1], s_red[1][1]), fmin(s_red[2][1], s_red[3][1]));
        row[2] = fmax(fmax(s_red[0][2], s_red[1][2]), fmax(s_red[2][2], s_red[3][2]));
    }
}

// One workgroup sums the slab in a fixed order: thread t the rows t, t + 256, ..., then a tree over the threads.
// out[5] = (n, min, max, mean, std): pass 0 writes the first four, pass 1 the last.
template <int PASS>
__global__ __launch_bounds__(PP_THREADS) void pp_moments_final_kernel(const double* __restrict__ slab, int blocks, int64_t n,
                                                                      double* __restrict__ out) {
    __shared__ double s_sum[PP_THREADS], s_lo[PP_THREADS], s_hi[PP_THREADS];
    const int t = threadIdx.x;
    double s = 0.0, lo = INFINITY, hi = -INFINITY;
    for (int i = t; i < blocks; i += PP_THREADS) {
        s += slab[(int64_t)i * 3];
        if (PASS == 0) lo = fmin(lo, slab[(int64_t)i * 3 + 1]), hi = fmax(hi, slab[(int64_t)i * 3 + 2]);
    }
    s_sum[t] = s, s_lo[t] = lo, s_hi[t] = hi;
    __syncthreads();
    for (int off = PP_THREADS / 2; off > 0; off >>= 1) {
        if (t < off) {
            s_sum[t] += s_sum[t + off];
            s_lo[t] = fmin(s_lo[t], s_lo[t + off]), s_hi[t] = fmax(s_hi[t], s_hi[t + off]);
        }
        __syncthreads();
    }
    if (t == 0) {
        if (PASS == 0) out[0] = (double)n, out[1] = s_lo[0], out[2] = s_hi[0], out[3] = s_sum[0] / (double)n;
        else out[4] = sqrt(s_sum[0] / (double)n);
    }
}

// ------------------------------------------------------------------------------------------------ entry points
extern "C" int ru3d_threshold_bbox(const float* image, int X, int Y, int Z, int C, float threshold, int32_t* box,
                                   int64_t* count, void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    PP_REQUIRE_SHAPE("threshold_bbox");
    RU3D_REQUIRE(C >= 1, "threshold_bbox: %d channels", C);
    RU3D_REQUIRE(image && box && count, "threshold_bbox: bad argument (null pointer)");
    RU3D_REQUIRE(threshold == threshold, "threshold_bbox: the threshold is not a number");
    hipStream_t st = as_stream(stream);
    const int n = X * Y * Z;
    pp_u64* cnt = (pp_u64*)count;
    hipLaunchKernelGGL(pp_bbox_init_kernel, dim3(1), dim3(64), 0, st, box, cnt);
    const bool vec = pp_aligned16(image) && C <= 4;
    const dim3 grid(pp_stream_blocks(vec ? (n + 3) / 4 : n)), block(PP_THREADS);
#define PP_BBOX(CT) hipLaunchKernelGGL(pp_bbox_kernel<CT>, grid, block, 0, st, image, Y, Z, C, n, threshold, box, cnt)
    if (!vec) PP_BBOX(0);
    else if (C == 1) PP_BBOX(1);
    else if (C == 2) PP_BBOX(2);
    else if (C == 3) PP_BBOX(3);
    else PP_BBOX(4);
#undef PP_BBOX
    return ru3d_check_launch("threshold_bbox");
}

static inline int pp_chunks(int64_t n) { return (int)((n + PP_CHUNK - 1) / PP_CHUNK); }

extern "C" size_t ru3d_masked_sample_workspace_bytes(int X, int Y, int Z) {
    if (!bv_shape_ok(X, Y, Z)) return 0;
    return bv_align((size_t)pp_chunks((int64_t)X * Y * Z) * sizeof(int));
}

extern "C" int ru3d_masked_sample(const float* image, int X, int Y, int Z, int C, int channel, const void* label,
                                  int label_dtype, int stride, float* out, int64_t capacity, int64_t* count, void* ws,
                                  size_t ws_bytes, void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    PP_REQUIRE_SHAPE("masked_sample");
    RU3D_REQUIRE(C >= 1 && channel >= 0 && channel < C, "masked_sample: channel %d of %d", channel, C);
    RU3D_REQUIRE(label_dtype == RU3D_LABEL_I64 || label_dtype == RU3D_LABEL_U8,
                 "masked_sample: label dtype code %d (RU3D_LABEL_I64 / RU3D_LABEL_U8)", label_dtype);
    RU3D_REQUIRE(stride >= 1, "masked_sample: stride %d (>= 1)", stride);
    RU3D_REQUIRE(label && count && ws && (image || !out), "masked_sample: bad argument (null pointer)");
    RU3D_REQUIRE(!out || capacity >= 1, "masked_sample: capacity %lld of the output buffer (>= 1)", (long long)capacity);
    RU3D_REQUIRE(ws_bytes >= ru3d_masked_sample_workspace_bytes(X, Y, Z), "masked_sample: workspace of %zu bytes, %zu needed",
                 ws_bytes, ru3d_masked_sample_workspace_bytes(X, Y, Z));
    hipStream_t st = as_stream(stream);
    const int n = X * Y * Z, chunks = pp_chunks(n);
    int* counts = (int*)ws;
    const dim3 grid(chunks), block(PP_THREADS);
    if (label_dtype == RU3D_LABEL_U8)
        hipLaunchKernelGGL(pp_fg_count_kernel<uint8_t>, grid, block, 0, st, (const uint8_t*)label, n, counts);
    else
        hipLaunchKernelGGL(pp_fg_count_kernel<int64_t>, grid, block, 0, st, (const int64_t*)label, n, counts);
    hipLaunchKernelGGL(pp_scan_kernel, dim3(1), dim3(BV_SCAN_THREADS), 0, st, counts, chunks, stride, (long long*)count);
    if (out) {
        if (label_dtype == RU3D_LABEL_U8)
            hipLaunchKernelGGL(pp_sample_scatter_kernel<uint8_t>, grid, block, 0, st, image, C, channel,
                               (const uint8_t*)label, n, stride, counts, out, (long long)capacity);
        else
            hipLaunchKernelGGL(pp_sample_scatter_kernel<int64_t>, grid, block, 0, st, image, C, channel,
                               (const int64_t*)label, n, stride, counts, out, (long long)capacity);
    }
    return ru3d_check_launch("masked_sample");
}

extern "C" size_t ru3d_order_stats_workspace_bytes(void) {
    return bv_align(sizeof(pp_select_state)) + bv_align((size_t)PP_PASSES * PP_MAX_RANKS * PP_BINS * sizeof(pp_u64));
}

extern "C" int ru3d_order_stats(const float* values, int64_t n, const int64_t* ranks, int num_ranks, float* out, void* ws,
                                size_t ws_bytes, void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    RU3D_REQUIRE(n >= 1 && n < ((int64_t)1 << 40), "order_stats: %lld values (1 .. 2^40 - 1)", (long long)n);
    RU3D_REQUIRE(num_ranks >= 1 && num_ranks <= PP_MAX_RANKS, "order_stats: %d ranks (1 .. %d)", num_ranks, PP_MAX_RANKS);
    RU3D_REQUIRE(values && ranks && out && ws, "order_stats: bad argument (null pointer)");
    RU3D_REQUIRE(((uintptr_t)values & 3) == 0, "order_stats: the values are not 4-byte aligned");
    pp_ranks first = {};
    for (int r = 0; r < num_ranks; r++) {
        RU3D_REQUIRE(ranks[r] >= 0 && ranks[r] < n, "order_stats: rank %lld of %lld values", (long long)ranks[r],
                     (long long)n);
        first.k[r] = ranks[r];
    }
    RU3D_REQUIRE(ws_bytes >= ru3d_order_stats_workspace_bytes(), "order_stats: workspace of %zu bytes, %zu needed", ws_bytes,
                 ru3d_order_stats_workspace_bytes());
    hipStream_t st = as_stream(stream);
    pp_select_state* state = (pp_select_state*)ws;
    pp_u64* hist = (pp_u64*)((char*)ws + bv_align(sizeof(pp_select_state)));
    const size_t table = (size_t)PP_MAX_RANKS * PP_BINS;
    if (hipMemsetAsync(hist, 0, PP_PASSES * table * sizeof(pp_u64), st) != hipSuccess)
        return ru3d_check_launch("order_stats (memset)");
    const dim3 grid(pp_stream_blocks((n + 3) / 4));
    for (int pass = 0; pass < PP_PASSES; pass++) {
        hipLaunchKernelGGL(pp_hist_kernel, grid, dim3(PP_THREADS), 0, st, values, n, pass, num_ranks,
                           (const pp_select_state*)state, hist + pass * table);
        hipLaunchKernelGGL(pp_select_kernel, dim3(1), dim3(PP_BINS), 0, st, pass, num_ranks, first, state,
                           (const pp_u64*)(hist + pass * table), out);
    }
    return ru3d_check_launch("order_stats");
}

extern "C" size_t ru3d_moments_workspace_bytes(void) { return bv_align((size_t)PP_MAX_BLOCKS * 3 * sizeof(double)); }

extern "C" int ru3d_moments(const float* values, int64_t n, double* out, void* ws, size_t ws_bytes, void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    RU3D_REQUIRE(n >= 1 && n < ((int64_t)1 << 40), "moments: %lld values (1 .. 2^40 - 1)", (long long)n);
    RU3D_REQUIRE(values && out && ws, "moments: bad argument (null pointer)");
    RU3D_REQUIRE(((uintptr_t)values & 3) == 0, "moments: the values are not 4-byte aligned");
    RU3D_REQUIRE(ws_bytes >= ru3d_moments_workspace_bytes(), "moments: workspace of %zu bytes, %zu needed", ws_bytes,
                 ru3d_moments_workspace_bytes());
    hipStream_t st = as_stream(stream);
    double* slab = (double*)ws;
    const unsigned blocks = pp_stream_blocks((n + 3) / 4);
    const dim3 grid(blocks), block(PP_THREADS);
    hipLaunchKernelGGL(pp_moments_partial_kernel<0>, grid, block, 0, st, values, n, (const double*)out, slab);
    hipLaunchKernelGGL(pp_moments_final_kernel<0>, dim3(1), block, 0, st, (const double*)slab, (int)blocks, n, out);
    hipLaunchKernelGGL(pp_moments_partial_kernel<1>, grid, block, 0, st, values, n, (const double*)out, slab);
    hipLaunchKernelGGL(pp_moments_final_kernel<1>, dim3(1), block, 0, st, (const double*)slab, (int)blocks, n, out);
    return ru3d_check_launch("moments");
}
