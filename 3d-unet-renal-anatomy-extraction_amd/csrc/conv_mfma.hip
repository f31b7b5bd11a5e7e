// bf16 MFMA implicit-GEMM convolution kernels for gfx950 (v_mfma_f32_32x32x16_bf16, fp32 accumulate).
//
// GEMM view of a 3x3x3 stride-1 conv on NDHWC data:  D[cout][voxel] = sum_{tap, ci} W[tap][cout][ci] * X[voxel+tap][ci]
//   A operand (rows = cout)   : weights, pre-packed in exact fragment order (one contiguous 1 KiB load per
//                               wave-instruction, served from L1/L2 - every workgroup reads the same weights)
//   B operand (cols = voxel)  : activations; a workgroup stages the (TD+2)x(TH+2)x(TW+2) halo tile of a
//                               32-channel chunk in LDS once and every tap reads its fragments from there with
//                               ds_read_b128 (voxel pitch 80 B = 64 B data + 16 B pad: conflict-free for a
//                               32-voxel W-run)
//   C/D                       : lane = voxel (l & 31), registers = 16 couts in groups of 4 consecutive channels
//                               -> 8-byte NDHWC stores, bias / residual fused in the epilogue.
// Workgroup: 256 threads = 4 waves, output tile TDxTHxTW = 256 voxels (8 MFMA column tiles, 2 per wave) x NT*32
// couts.  2 workgroups per CU (LDS <= 65 KB) so one group's staging overlaps the other's MFMA phase.
#include "common.h"
#include "conv.h"

#include <type_traits>

namespace RU3D_NS {

#define MF_PITCH 40  // bf16 elements per staged voxel (32 data + 8 pad) = 80 bytes

// ---------------------------------------------------------------------------------------------------------
// Weight packing: dst[((tap * KS + ks) * NTT + nt) * 64 + lane][j] = W[tap][co = nt*32 + (lane&31)][ci = ks*16 + 8*(lane>>5) + j]
// (KS = cin/16 k-steps, NTT = cout/32).  src index = co*s_o + ci*s_i + tap.
__global__ void pack_mfma_kernel(const float* __restrict__ src, bf16* __restrict__ dst, int cin, int cout, int taps,
                                 int64_t s_o, int64_t s_i) {
    const int KS = cin / 16, NTT = cout / 32;
    const int64_t total = (int64_t)taps * KS * NTT * 64 * 8;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int j = (int)(i & 7);
        const int lane = (int)((i >> 3) & 63);
        int64_t t = i >> 9;
        const int nt = (int)(t % NTT);
        t /= NTT;
        const int ks = (int)(t % KS);
        const int tap = (int)(t / KS);
        const int co = nt * 32 + (lane & 31);
        const int ci = ks * 16 + 8 * (lane >> 5) + j;
        dst[i] = (bf16)src[co * s_o + ci * s_i + tap];
    }
}

size_t mfma_packed_bytes(int cin, int cout, int taps) { return (size_t)taps * cin * cout * 2; }

int pack_mfma_launch(const float* src, void* dst, int cin, int cout, int taps, int64_t s_o, int64_t s_i, int flip,
                     hipStream_t st) {
    (void)flip;
    const int64_t total = (int64_t)taps * cin * cout;
    int blocks = (int)((total + 255) / 256);
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(pack_mfma_kernel, dim3(blocks), dim3(256), 0, st, src, (bf16*)dst, cin, cout, taps, s_o, s_i);
    return ru3d_check_launch("pack_mfma");
}

// Which (shape, dtype) combinations take the MFMA path.  Must agree between ru3d_pack_weight and the launchers.
bool mfma_conv_eligible(int cin, int cout, int k, int dtype, int y_dtype) {
    return dtype == RU3D_BF16 && y_dtype == RU3D_BF16 && (k == 1 || k == 3) && (cin % 16) == 0 && (cout % 32) == 0;
}

// ---------------------------------------------------------------------------------------------------------
struct MfmaConvArgs {
    const bf16* x;
    const bf16x8* w;
    const float* bias;
    const bf16* res;
    bf16* y;
    int N, D, H, W;        // stride 1, pad 1: input extents == output extents
    int Cin, Cout, ldx, ldy, ldr;
    int tiles_d, tiles_h, tiles_w;
    int flip;
    int nblk;              // spatial tiles * N (grid.x)
    float* stat_slab;      // optional: per-(workgroup, wave, n, cout) {sum, sum of squares} of the stored outputs
    float* part;           // split-K (deep levels): fp32 partial outputs [blockIdx.z][voxel][Cout], no bias/residual
    int ksplit;            // number of 32-channel chunk groups (gridDim.z); 1 = none
    void* ws;              // caller-owned workspace for the split-K partials (may be null: no split-K)
    size_t ws_bytes;
    int* defer_ks;         // host side: leave the split-K partials in ws un-summed and report their count here (0 = y is final)
};

// T1 (bijective): consecutive hardware block ids round-robin over the 8 XCDs; give each XCD a contiguous
// run of tiles so that halo re-reads between neighbouring tiles hit the same L2.  Speed only.
__device__ __forceinline__ int xcd_remap(int bid, int nblk) {
    const int q = nblk >> 3, r = nblk & 7, xcd = bid & 7;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
}

// MT = MFMA column tiles (32 voxels) per wave: 2 for the large levels (256-voxel tile), 1 for the deep,
// spatially small levels where more, smaller workgroups are needed to fill 256 CUs.
// WD = depth (in (tap, k-step) steps) of the register ring that prefetches weight fragments: the loads of step
// s + WD are issued right after the MFMAs of step s, so ~WD*MT*NT MFMAs (>= 500 cycles) cover an L2 hit.
template <int TD, int TH, int TW, int MT, int NT>
__global__ __launch_bounds__(256, 2) void conv3_s1_mfma_kernel(MfmaConvArgs a) {
    constexpr int HD = TD + 2, HH = TH + 2, WW = TW + 2;
    constexpr int HV = HD * HH * WW;
    constexpr int WD = (MT * NT >= 4) ? 6 : 12;   // weight-fragment ring depth (steps)
    constexpr int XD = 3;                          // activation-fragment ring depth (steps)
    constexpr int S = 54;   // 27 taps x 2 k-steps per 32-channel chunk
    static_assert(TD * TH * TW == 128 * MT, "tile must hold 128*MT voxels");
    static_assert(HV * MF_PITCH * 2 <= 65536, "halo tile must leave room for 2 workgroups per CU");
    __shared__ __attribute__((aligned(16))) bf16 lds[HV * MF_PITCH];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // (round 4: a 1-D launch in which every XCD owned a fixed slice of the cout tiles - its L2 holding 1/8 of the weight,
    // every weight byte leaving HBM once - changed nothing: 28.2 vs 28.4 us at 512 -> 512 on 8^3, 37.9 vs 37.9 at 16^3,
    // profiles/r04_deep_level_convs.txt.  Where the weight bytes are served from is not what bounds these kernels; the
    // CUs' L1 path is: four waves x 1 KB of weight fragments per 2 MFMAs.)
    const int by = blockIdx.y, bz = blockIdx.z, gz = gridDim.z;
    int tile = xcd_remap(blockIdx.x, a.nblk);
    const int tw_i = tile % a.tiles_w;
    tile /= a.tiles_w;
    const int th_i = tile % a.tiles_h;
    tile /= a.tiles_h;
    const int td_i = tile % a.tiles_d;
    const int n = tile / a.tiles_d;
    const int d0 = td_i * TD, h0 = th_i * TH, w0 = tw_i * TW;
    const int co_blk = by * (NT * 32);
    const int NTT = a.Cout / 32, KS = a.Cin / 16;

    // this lane's output voxels (one per MFMA column tile owned by the wave)
    int hv0[MT], od[MT], oh[MT], ow[MT];
#pragma unroll
    for (int m = 0; m < MT; m++) {
        const int f = (wave * MT + m) * 32 + (lane & 31);
        const int tdl = f / (TH * TW), thl = (f / TW) % TH, twl = f % TW;
        od[m] = d0 + tdl;
        oh[m] = h0 + thl;
        ow[m] = w0 + twl;
        hv0[m] = ((tdl * HH + thl) * WW + twl) * MF_PITCH + (lane >> 5) * 8;  // + k-half of the fragment
    }

    f32x16 acc[MT][NT];
#pragma unroll
    for (int m = 0; m < MT; m++)
#pragma unroll
        for (int t = 0; t < NT; t++)
#pragma unroll
            for (int i = 0; i < 16; i++) acc[m][t][i] = 0.f;

    const bf16x8* wbase = a.w + (int64_t)by * NT * 64 + lane;
    const int nchunks = a.Cin / 32;
    // split-K: blockIdx.z owns a contiguous run of 32-channel chunks and writes an fp32 partial
    const int ch_lo = (nchunks * bz) / gz, ch_hi = (nchunks * (bz + 1)) / gz;
    for (int ch = ch_lo; ch < ch_hi; ch++) {
        // ---- weight ring prologue (independent of LDS: its latency hides under the staging below)
        bf16x8 wq[WD][NT];
#pragma unroll
        for (int s = 0; s < WD; s++) {
            const int tap = s >> 1, kc = s & 1;
            const int wtap = a.flip ? 26 - tap : tap;
#pragma unroll
            for (int t = 0; t < NT; t++) wq[s][t] = wbase[((int64_t)(wtap * KS + ch * 2 + kc) * NTT + t) * 64];
        }
        // ---- stage the halo tile of channels [32 ch, 32 ch + 32): all loads first, then all LDS writes
        constexpr int NIT = (HV * 4 + 255) / 256;
        bf16x8 stage[NIT];
#pragma unroll
        for (int i = 0; i < NIT; i++) {
            const int c = tid + i * 256;
            const int hv = c >> 2, part = c & 3;
            const int zw = hv % WW, zh = (hv / WW) % HH, zd = hv / (WW * HH);
            const int gd = d0 + zd - 1, gh = h0 + zh - 1, gw = w0 + zw - 1;
            bf16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
            if (c < HV * 4 && gd >= 0 && gd < a.D && gh >= 0 && gh < a.H && gw >= 0 && gw < a.W)
                v = *reinterpret_cast<const bf16x8*>(a.x + ((((int64_t)n * a.D + gd) * a.H + gh) * a.W + gw) * a.ldx +
                                                     ch * 32 + part * 8);
            stage[i] = v;
        }
        if (ch > ch_lo) __syncthreads();  // everyone done reading the previous chunk
#pragma unroll
        for (int i = 0; i < NIT; i++) {
            const int c = tid + i * 256;
            if (c < HV * 4) *reinterpret_cast<bf16x8*>(&lds[(c >> 2) * MF_PITCH + (c & 3) * 8]) = stage[i];
        }
        __syncthreads();
        // ---- 27 taps x 2 k-steps of 16 channels.  Software pipeline pinned with sched_barrier: the LDS
        // fragments of step s+1 and the weight fragments of step s+WD are issued before / right after the
        // MFMAs of step s (hipcc otherwise sinks every load to just before its use: vmcnt(1) per step).
        // activation fragments: ring of XD steps read ahead from LDS (ds_read_b128 latency under load is
        // well above one MFMA pair, so a 1-step lookahead still exposes it)
        bf16x8 xq[XD][MT];
#pragma unroll
        for (int s = 0; s < XD; s++) {
            const int tap0 = s >> 1, kc0 = s & 1;
            const int toff0 = (((tap0 / 9) * HH + (tap0 / 3) % 3) * WW + tap0 % 3) * MF_PITCH;
#pragma unroll
            for (int m = 0; m < MT; m++) xq[s][m] = *reinterpret_cast<const bf16x8*>(&lds[hv0[m] + toff0 + kc0 * 16]);
        }
#pragma unroll
        for (int s = 0; s < S; s++) {
#pragma unroll
            for (int t = 0; t < NT; t++)
#pragma unroll
                for (int m = 0; m < MT; m++)
                    acc[m][t] = RU3D_MFMA_32X32X16(wq[s % WD][t], xq[s % XD][m], acc[m][t], 0, 0, 0);
            if (s + XD < S) {
                const int tap1 = (s + XD) >> 1, kc1 = (s + XD) & 1;
                const int toff1 = (((tap1 / 9) * HH + (tap1 / 3) % 3) * WW + tap1 % 3) * MF_PITCH;
#pragma unroll
                for (int m = 0; m < MT; m++)
                    xq[s % XD][m] = *reinterpret_cast<const bf16x8*>(&lds[hv0[m] + toff1 + kc1 * 16]);
            }
            if (s + WD < S) {
                const int tap2 = (s + WD) >> 1, kc2 = (s + WD) & 1;
                const int wtap2 = a.flip ? 26 - tap2 : tap2;
#pragma unroll
                for (int t = 0; t < NT; t++)
                    wq[s % WD][t] = wbase[((int64_t)(wtap2 * KS + ch * 2 + kc2) * NTT + t) * 64];
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }

    // ---- epilogue: lane = voxel, 16 couts per accumulator in 4 groups of 4 consecutive channels
#pragma unroll
    for (int m = 0; m < MT; m++) {
        if (od[m] >= a.D || oh[m] >= a.H || ow[m] >= a.W) continue;
        const int64_t vox = (((int64_t)n * a.D + od[m]) * a.H + oh[m]) * a.W + ow[m];
        if (a.part) {
            float* pp = a.part + ((int64_t)bz * ((int64_t)a.N * a.D * a.H * a.W) + vox) * a.Cout;
#pragma unroll
            for (int t = 0; t < NT; t++)
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    f32x4 v;
#pragma unroll
                    for (int i = 0; i < 4; i++) v[i] = acc[m][t][q * 4 + i];
                    *reinterpret_cast<f32x4*>(pp + co_blk + t * 32 + 8 * q + 4 * (lane >> 5)) = v;
                }
            continue;
        }
#pragma unroll
        for (int t = 0; t < NT; t++) {
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int c0 = co_blk + t * 32 + 8 * q + 4 * (lane >> 5);
                float v[4];
#pragma unroll
                for (int i = 0; i < 4; i++) v[i] = acc[m][t][q * 4 + i];
                if (a.bias) {
                    const f32x4 b = *reinterpret_cast<const f32x4*>(a.bias + c0);
#pragma unroll
                    for (int i = 0; i < 4; i++) v[i] += b[i];
                }
                if (a.res) {
                    float r[4];
                    load_vec<bf16, 4>(a.res + vox * a.ldr + c0, r);
#pragma unroll
                    for (int i = 0; i < 4; i++) v[i] += r[i];
                }
                store_vec<bf16, 4>(a.y + vox * a.ldy + c0, v);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// Producer/consumer form of the same conv for the large levels (>= 2 tiles per CU):
//   * persistent workgroup of 8 waves, one per CU: waves 0-3 CONSUME (MFMA loop + epilogue, weights through
//     their own vmcnt-tracked register ring), waves 4-7 PRODUCE (global -> registers -> LDS staging of the
//     NEXT (tile, 32-channel chunk) item into the other of two LDS halo buffers).  vmcnt is per wave and
//     in-order, so keeping the long-latency halo loads out of the consumer waves is what lets the weight ring
//     run with counted waits.  One s_barrier per item hands the buffers over.
//   * the producers' per-piece global / LDS offsets are tile-invariant and computed once; interior tiles
//     skip the bounds checks.
//   * work is dealt XCD-contiguously: the blocks that share an XCD walk a contiguous run of tiles, so the halo
//     re-reads of neighbouring tiles meet in that XCD's L2.
// MT = column tiles per consumer wave (tile = 128*MT voxels); the 512-voxel form is conv3_s1_pc4_kernel below.
template <int TD, int TH, int TW, int MT, int NT>
__global__ __launch_bounds__(512, 2) void conv3_s1_pc_kernel(MfmaConvArgs a) {
    constexpr int PITCH = MF_PITCH;
    constexpr int HD = TD + 2, HH = TH + 2, WW = TW + 2;
    constexpr int HV = HD * HH * WW;
    // ring depths: ~700 cycles of MFMA work between a weight load and its use, ~2 MFMA groups for LDS reads
    constexpr int WD = (768 + 32 * MT * NT - 1) / (32 * MT * NT);
    constexpr int XD = (MT >= 4) ? 2 : 3;
    constexpr int S = 54;
    constexpr int NIT = (HV * 4 + 255) / 256;
    static_assert(TD * TH * TW == 128 * MT, "tile must hold 128*MT voxels");
    static_assert((2 * HV * PITCH + 4 * MT * 32 * MF_PITCH) * 2 <= 160 * 1024, "two halo buffers must fit in LDS");
    __shared__ __attribute__((aligned(16))) bf16 lds[2 * HV * PITCH + 4 * MT * 32 * MF_PITCH];   // 2 halo buffers + epilogue patches
    // element offset of 16-byte piece `p` of halo voxel `hv`
    auto piece_off = [](int hv, int p) { return hv * MF_PITCH + (p << 3); };

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool producer = wave >= 4;
    const int NTT = a.Cout / 32, KS = a.Cin / 16;
    const int nchunks = a.Cin / 32;

    // ---- this workgroup's tiles: XCD-contiguous run, strided by the number of workgroups on that XCD label
    const int G = gridDim.x, b = blockIdx.x;
    const int L = G < 8 ? G : 8;                             // XCD labels in use
    const int xcd = b % L, idx = b / L;
    const int gx = (G - xcd + L - 1) / L;                    // workgroups with this label
    const int t_begin = (int)(((int64_t)a.nblk * xcd) / L), t_end = (int)(((int64_t)a.nblk * (xcd + 1)) / L);
    const int my_tiles = (t_begin + idx < t_end) ? (t_end - t_begin - idx + gx - 1) / gx : 0;
    const int nitems = my_tiles * nchunks;

    auto tile_origin = [&](int tile, int& n, int& d0, int& h0, int& w0) {
        const int tw_i = tile % a.tiles_w;
        tile /= a.tiles_w;
        const int th_i = tile % a.tiles_h;
        tile /= a.tiles_h;
        const int td_i = tile % a.tiles_d;
        n = tile / a.tiles_d;
        d0 = td_i * TD;
        h0 = th_i * TH;
        w0 = tw_i * TW;
    };

    if (producer) {
        // ------------------------------------------------------------------ producer waves
        const int pt = tid - 256;
        const int part = pt & 3;                 // c = pt + 256 i: the 16-byte piece index is fixed per thread
        int rel[NIT], zz[NIT];
#pragma unroll
        for (int i = 0; i < NIT; i++) {
            const int c = pt + i * 256;
            const int hv = (c < HV * 4) ? (c >> 2) : 0;
            const int zw = hv % WW, zh = (hv / WW) % HH, zd = hv / (WW * HH);
            rel[i] = ((zd * a.H + zh) * a.W + zw) * a.ldx + part * 8;
            zz[i] = (c < HV * 4) ? (zd | (zh << 8) | (zw << 16)) : -1;
        }
        constexpr int HALF = (NIT + 1) / 2;       // two batches of loads keep the staging registers at 4*HALF
        for (int it = 0; it <= nitems; it++) {
            if (it < nitems) {
                const int tile = t_begin + idx + (it / nchunks) * gx, ch = it % nchunks;
                int n, d0, h0, w0;
                tile_origin(tile, n, d0, h0, w0);
                const bf16* src = a.x + ((((int64_t)n * a.D + (d0 - 1)) * a.H + (h0 - 1)) * a.W + (w0 - 1)) * a.ldx + ch * 32;
                const bool interior = d0 >= 1 && d0 + TD + 1 <= a.D && h0 >= 1 && h0 + TH + 1 <= a.H && w0 >= 1 &&
                                      w0 + TW + 1 <= a.W;
                bf16* dst = lds + (it & 1) * (HV * PITCH);
#pragma unroll
                for (int hb = 0; hb < 2; hb++) {
                    bf16x8 stage[HALF];
#pragma unroll
                    for (int j = 0; j < HALF; j++) {
                        const int i = hb * HALF + j;
                        bf16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
                        if (i < NIT) {
                            bool ok = zz[i] >= 0;
                            if (!interior) {
                                const int gd = d0 - 1 + (zz[i] & 255), gh = h0 - 1 + ((zz[i] >> 8) & 255),
                                          gw = w0 - 1 + ((zz[i] >> 16) & 255);
                                ok = ok && gd >= 0 && gd < a.D && gh >= 0 && gh < a.H && gw >= 0 && gw < a.W;
                            }
                            if (ok) v = *reinterpret_cast<const bf16x8*>(src + rel[i]);
                        }
                        stage[j] = v;
                    }
#pragma unroll
                    for (int j = 0; j < HALF; j++) {
                        const int i = hb * HALF + j;
                        if (i < NIT && zz[i] >= 0) {
                            const int hv = (((zz[i] & 255) * HH) + ((zz[i] >> 8) & 255)) * WW + ((zz[i] >> 16) & 255);
                            *reinterpret_cast<bf16x8*>(dst + piece_off(hv, part)) = stage[j];
                        }
                    }
                }
            }
            __syncthreads();
        }
        return;
    }

    // ---------------------------------------------------------------------- consumer waves
    const int co_blk = blockIdx.y * (NT * 32);
    int hvl[MT];
#pragma unroll
    for (int m = 0; m < MT; m++) {
        const int f = (wave * MT + m) * 32 + (lane & 31);
        hvl[m] = ((f / (TH * TW)) * HH + (f / TW) % TH) * WW + f % TW;   // halo voxel index of tap (0,0,0)
    }
    const bf16x8* wbase = a.w + (int64_t)blockIdx.y * NT * 64 + lane;
    f32x16 acc[MT][NT];
    // bias of this lane's 16 couts per cout tile, loaded once (the epilogue must not wait on global loads)
    f32x4 bq[NT][4];
#pragma unroll
    for (int t = 0; t < NT; t++)
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
            bq[t][q] = a.bias ? *reinterpret_cast<const f32x4*>(a.bias + co_blk + t * 32 + 8 * q + 4 * (lane >> 5)) : z4;
        }
    // fused InstanceNorm statistics: running {sum, sum^2} of this wave's stored values for the sample `cur_n`
    float st1[NT][8], st2[NT][8];
    int cur_n = -1;
    if (a.stat_slab)
        ru3d_clear_own_slab_rows(a.stat_slab, (int64_t)(blockIdx.y * gridDim.x + blockIdx.x) * 4 + wave, a.N, NT * 32 * 2);
    auto stat_flush = [&]() {
        if (!a.stat_slab || cur_n < 0) return;
        const int blk = blockIdx.y * gridDim.x + blockIdx.x;
        float* dst = a.stat_slab + ((((int64_t)blk * 4 + wave) * a.N + cur_n) * (NT * 32)) * 2;
#pragma unroll
        for (int t = 0; t < NT; t++)
#pragma unroll
            for (int i = 0; i < 8; i++) {
                float s1 = st1[t][i], s2 = st2[t][i];
#pragma unroll
                for (int o = 4; o < 64; o <<= 1) {   // lanes that share (lane & 3) hold the same 8 channels
                    s1 += __shfl_xor(s1, o, 64);
                    s2 += __shfl_xor(s2, o, 64);
                }
                if (lane < 4) {
                    const int c = t * 32 + lane * 8 + i;
                    dst[c * 2] = s1;
                    dst[c * 2 + 1] = s2;
                }
            }
    };

    for (int it = 0; it <= nitems; it++) {
        if (it >= 1) {
            const int item = it - 1;
            const int tile = t_begin + idx + (item / nchunks) * gx, ch = item % nchunks;
            const bf16* buf = lds + (item & 1) * (HV * PITCH);
            const int ph = lane >> 5;   // k-half of the fragment
            if (ch == 0) {
#pragma unroll
                for (int m = 0; m < MT; m++)
#pragma unroll
                    for (int t = 0; t < NT; t++)
#pragma unroll
                        for (int i = 0; i < 16; i++) acc[m][t][i] = 0.f;
            }
            bf16x8 wq[WD][NT];
#pragma unroll
            for (int s = 0; s < WD; s++) {
                const int tap = s >> 1, kc = s & 1;
                const int wtap = a.flip ? 26 - tap : tap;
#pragma unroll
                for (int t = 0; t < NT; t++) wq[s][t] = wbase[((int64_t)(wtap * KS + ch * 2 + kc) * NTT + t) * 64];
            }
            bf16x8 xq[XD][MT];
#pragma unroll
            for (int s = 0; s < XD; s++) {
                const int tap0 = s >> 1, kc0 = s & 1;
                const int toff0 = ((tap0 / 9) * HH + (tap0 / 3) % 3) * WW + tap0 % 3;
#pragma unroll
                for (int m = 0; m < MT; m++)
                    xq[s][m] = *reinterpret_cast<const bf16x8*>(&buf[piece_off(hvl[m] + toff0, kc0 * 2 + ph)]);
            }
#pragma unroll
            for (int s = 0; s < S; s++) {
#pragma unroll
                for (int t = 0; t < NT; t++)
#pragma unroll
                    for (int m = 0; m < MT; m++)
                        acc[m][t] = RU3D_MFMA_32X32X16(wq[s % WD][t], xq[s % XD][m], acc[m][t], 0, 0, 0);
                if (s + XD < S) {
                    const int tap1 = (s + XD) >> 1, kc1 = (s + XD) & 1;
                    const int toff1 = ((tap1 / 9) * HH + (tap1 / 3) % 3) * WW + tap1 % 3;
#pragma unroll
                    for (int m = 0; m < MT; m++)
                        xq[s % XD][m] = *reinterpret_cast<const bf16x8*>(&buf[piece_off(hvl[m] + toff1, kc1 * 2 + ph)]);
                }
                if (s + WD < S) {
                    const int tap2 = (s + WD) >> 1, kc2 = (s + WD) & 1;
                    const int wtap2 = a.flip ? 26 - tap2 : tap2;
#pragma unroll
                    for (int t = 0; t < NT; t++)
                        wq[s % WD][t] = wbase[((int64_t)(wtap2 * KS + ch * 2 + kc2) * NTT + t) * 64];
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            if (ch == nchunks - 1) {
                // ---- epilogue through a wave-private LDS patch: the accumulator layout (lane = voxel, 4 couts
                // per 8 bytes) would give 8-byte stores scattered over 32 rows per instruction (store-issue
                // bound); transposed through LDS every lane stores 16 bytes and a wave-instruction covers 16
                // whole 64-byte channel rows.  Bias is added before, the residual after the transpose.
                int n, d0, h0, w0;
                tile_origin(tile, n, d0, h0, w0);
                if (a.stat_slab && n != cur_n) {
                    stat_flush();
                    cur_n = n;
#pragma unroll
                    for (int t = 0; t < NT; t++)
#pragma unroll
                        for (int i = 0; i < 8; i++) st1[t][i] = st2[t][i] = 0.f;
                }
                bf16* est = lds + 2 * HV * PITCH + wave * (MT * 32 * MF_PITCH);
#pragma unroll
                for (int t = 0; t < NT; t++) {
#pragma unroll
                    for (int m = 0; m < MT; m++) {
#pragma unroll
                        for (int q = 0; q < 4; q++) {
                            const int cl = 8 * q + 4 * (lane >> 5);
                            float v[4];
#pragma unroll
                            for (int i = 0; i < 4; i++) v[i] = acc[m][t][q * 4 + i];
#pragma unroll
                            for (int i = 0; i < 4; i++) v[i] += bq[t][q][i];
                            store_vec<bf16, 4>(est + (m * 32 + (lane & 31)) * MF_PITCH + cl, v);
                        }
                    }
#pragma unroll
                    for (int r = 0; r < 2 * MT; r++) {
                        const int row = (lane >> 2) + 16 * r, part = lane & 3;
                        const int f = wave * (MT * 32) + row;
                        const int od = d0 + f / (TH * TW), oh = h0 + (f / TW) % TH, ow = w0 + f % TW;
                        float v[8];
                        load_vec<bf16, 8>(est + row * MF_PITCH + part * 8, v);
                        if (od < a.D && oh < a.H && ow < a.W) {
                            const int64_t vox = (((int64_t)n * a.D + od) * a.H + oh) * a.W + ow;
                            const int c0 = co_blk + t * 32 + part * 8;
                            if (a.stat_slab) {
#pragma unroll
                                for (int i = 0; i < 8; i++) {
                                    st1[t][i] += v[i];
                                    st2[t][i] = fmaf(v[i], v[i], st2[t][i]);
                                }
                            }
                            if (a.res) {
                                float rr[8];
                                load_vec<bf16, 8>(a.res + vox * a.ldr + c0, rr);
#pragma unroll
                                for (int i = 0; i < 8; i++) v[i] += rr[i];
                            }
                            store_vec<bf16, 8>(a.y + vox * a.ldy + c0, v);
                        }
                    }
                }
            }
        }
        __syncthreads();
    }
    stat_flush();
}

// ---------------------------------------------------------------------------------------------------------
// pc4: the producer/consumer kernel with 4 voxel tiles x 2 cout tiles of accumulators per consumer wave.
// Why (profiles/r04_pc_ablation.txt): with 2 x 2 tiles per wave every v_mfma_32x32x16 needs 512 B of weights through
// the CU's vector L1 (64 B/clk) and 512 B of activations out of LDS; four consumer waves at the MFMA rate ask the L1
// for exactly its peak, so the weight loads, the producers' halo loads and the MFMAs end up in series: 71 us where
// the MFMAs alone need 23-27 us (weight reloads removed: -15 us, producers' global loads removed: -12 us).  Here
//   * a consumer wave owns a 128-voxel x 64-cout block: 8 accumulators (128 AGPRs), a weight fragment serves four
//     MFMAs: half the L1 bytes per MFMA, the same LDS bytes;
//   * channel chunks of 16 (one MFMA k-step, 27 steps per item) so that two 512-voxel halo buffers fit: 32-byte voxel
//     slots, rows padded from 34 to 40 slots so that the slot's 16-byte halves can be XOR-swapped by bit 2 of the W
//     position alone (a ds_read_b128 of 32 consecutive voxels then touches every bank equally, for every tap offset)
//     and every fragment address is one of three per-lane bases + an immediate;
//   * the halo is moved by LDS-DMA (no staging registers, out-of-volume pieces come back as zeros through the buffer
//     range check), issued by the producer waves one item ahead; producers are the only waves that wait for it;
//   * the weight ring runs across item boundaries (27 = 9 x 3 steps, ring depth 3), so a new item starts with its
//     first fragments already in registers;
//   * barriers wait for LDS traffic only (lgkmcnt): a consumer's weight loads stay in flight across them;
//   * InstanceNorm statistics are kept in LDS between tiles (wave-private rows), not in registers.
// Tile: 4 x 4 x 32 voxels (wave = D plane, accumulator m = H row, lane = W position).
template <int WD>
__global__ __launch_bounds__(512, 2) void conv3_s1_pc4_kernel(MfmaConvArgs a) {
    constexpr int TD = 4, TH = 4, TW = 32, MT = 4, NT = 2;
    constexpr int HH = TH + 2, HD = TD + 2, WW = TW + 2, WWP = 40;
    constexpr int SLOTS = HD * HH * WWP;              // 32-byte voxel slots of one halo buffer (pads included)
    constexpr int BUF = SLOTS * 16;                   // bf16 elements
    constexpr int NCH = (SLOTS * 2) / 64;             // 1 KB DMA chunks per buffer
    constexpr int NDMA = (NCH + 3) / 4;               // per producer wave
    constexpr int S = 27, XD = 2;
    constexpr int OOBV = (int)0x80000000;
    static_assert((SLOTS * 2) % 64 == 0 && S % WD == 0, "whole DMA chunks; the ring must close over an item");
    __shared__ __attribute__((aligned(1024))) bf16 lds[2 * BUF + 4 * MT * 32 * MF_PITCH];
    __shared__ float statl[4][NT * 32 * 2];
    __shared__ __attribute__((aligned(16))) float biasl[NT * 32];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool producer = wave >= 4;
    const int NTT = a.Cout / 32, KS = a.Cin / 16;
    const int nchunks = KS;

    const int G = gridDim.x, b = blockIdx.x;
    const int L = G < 8 ? G : 8;
    const int xcd = b % L, idx = b / L;
    const int gx = (G - xcd + L - 1) / L;
    const int t_begin = (int)(((int64_t)a.nblk * xcd) / L), t_end = (int)(((int64_t)a.nblk * (xcd + 1)) / L);
    const int my_tiles = (t_begin + idx < t_end) ? (t_end - t_begin - idx + gx - 1) / gx : 0;
    const int nitems = my_tiles * nchunks;

    auto tile_origin = [&](int tile, int& n, int& d0, int& h0, int& w0) {
        const int tw_i = tile % a.tiles_w;
        tile /= a.tiles_w;
        const int th_i = tile % a.tiles_h;
        tile /= a.tiles_h;
        const int td_i = tile % a.tiles_d;
        n = tile / a.tiles_d;
        d0 = td_i * TD;
        h0 = th_i * TH;
        w0 = tw_i * TW;
    };

    if (producer) {
        // ------------------------------------------------------------------ producer waves: LDS-DMA of the next item
        const int pw = wave - 4;
        int rel[NDMA], zz[NDMA];
#pragma unroll
        for (int i = 0; i < NDMA; i++) {
            const int piece = (i * 4 + pw) * 64 + lane;            // 16-byte piece of the buffer this lane fills
            const int slot = piece >> 1;
            const int zw = slot % WWP, zh = (slot / WWP) % HH, zd = slot / (WWP * HH);
            const bool valid = (i * 4 + pw) < NCH && zw < WW;
            const int part = (piece & 1) ^ ((zw >> 2) & 1);        // which half of the voxel's 32 bytes lives here
            rel[i] = valid ? (((zd * a.H + zh) * a.W + zw) * a.ldx + part * 8) * 2 : OOBV;
            zz[i] = valid ? (zd | (zh << 8) | (zw << 16)) : -1;
        }
        const int64_t sample_elems = (int64_t)a.D * a.H * a.W * a.ldx;
        for (int it = 0; it <= nitems; it++) {
            if (it < nitems) {
                const int tile = t_begin + idx + (it / nchunks) * gx, ch = it % nchunks;
                int n, d0, h0, w0;
                tile_origin(tile, n, d0, h0, w0);
                const ru3d_i32x4 rsrc = ru3d_buffer_rsrc(a.x + n * sample_elems, (int)(sample_elems * 2));
                const int base = ((((d0 - 1) * a.H + (h0 - 1)) * a.W + (w0 - 1)) * a.ldx + ch * 16) * 2;
                const bool interior = d0 >= 1 && d0 + TD + 1 <= a.D && h0 >= 1 && h0 + TH + 1 <= a.H && w0 >= 1 &&
                                      w0 + TW + 1 <= a.W;
                const bf16* dst = lds + (it & 1) * BUF;
#pragma unroll
                for (int i = 0; i < NDMA; i++) {
                    if ((i * 4 + pw) < NCH) {
                        int off = zz[i] >= 0 ? base + rel[i] : OOBV;
                        if (!interior && zz[i] >= 0) {
                            const int gd = d0 - 1 + (zz[i] & 255), gh = h0 - 1 + ((zz[i] >> 8) & 255),
                                      gw = w0 - 1 + ((zz[i] >> 16) & 255);
                            if (!(gd >= 0 && gd < a.D && gh >= 0 && gh < a.H && gw >= 0 && gw < a.W)) off = OOBV;
                        }
                        ru3d_lds_dma16(rsrc, dst + (i * 4 + pw) * 512, off);
                    }
                }
            }
            asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
        }
        return;
    }

    // ---------------------------------------------------------------------- consumer waves
    const int co_blk = blockIdx.y * (NT * 32);
    const int ph = lane >> 5, wl = lane & 31;
    int xb[3];      // element offset of this lane's fragment piece for the three W offsets of a tap (wave's D plane)
#pragma unroll
    for (int tw = 0; tw < 3; tw++) {
        const int zw = wl + tw;
        xb[tw] = ((wave * HH) * WWP + zw) * 16 + ((ph ^ ((zw >> 2) & 1)) << 3);
    }
    const bf16x8* wbase = a.w + (int64_t)blockIdx.y * NT * 64 + lane;
    if (wave == 0) biasl[lane] = a.bias ? a.bias[co_blk + lane] : 0.f;
    statl[wave][lane] = 0.f;
    statl[wave][64 + lane] = 0.f;
    int cur_n = -1;
    if (a.stat_slab)
        ru3d_clear_own_slab_rows(a.stat_slab, (int64_t)(blockIdx.y * gridDim.x + blockIdx.x) * 4 + wave, a.N, NT * 32 * 2);
    auto stat_flush = [&]() {       // this wave's LDS sums -> its slab row of sample cur_n
        if (!a.stat_slab || cur_n < 0) return;
        const int blk = blockIdx.y * gridDim.x + blockIdx.x;
        float* dst = a.stat_slab + ((((int64_t)blk * 4 + wave) * a.N + cur_n) * (NT * 32)) * 2;
        dst[lane] = statl[wave][lane];
        dst[64 + lane] = statl[wave][64 + lane];
        statl[wave][lane] = 0.f;
        statl[wave][64 + lane] = 0.f;
    };

    f32x16 acc[MT][NT];
    bf16x8 wq[WD][NT];
#pragma unroll
    for (int s = 0; s < WD; s++) {      // the ring's first fragments: (tap s, chunk 0)
        const int wtap = a.flip ? 26 - s : s;
#pragma unroll
        for (int t = 0; t < NT; t++) wq[s][t] = wbase[((int64_t)(wtap * KS) * NTT + t) * 64];
    }

    for (int it = 0; it <= nitems; it++) {
        if (it >= 1) {
            const int item = it - 1;
            const int tile = t_begin + idx + (item / nchunks) * gx, ch = item % nchunks;
            const int chn = ch + 1 == nchunks ? 0 : ch + 1;
            const bf16* buf = lds + (item & 1) * BUF;
            if (ch == 0) {
#pragma unroll
                for (int m = 0; m < MT; m++)
#pragma unroll
                    for (int t = 0; t < NT; t++)
#pragma unroll
                        for (int i = 0; i < 16; i++) acc[m][t][i] = 0.f;
            }
            bf16x8 xq[XD][MT];
#pragma unroll
            for (int s = 0; s < XD; s++)
#pragma unroll
                for (int m = 0; m < MT; m++)
                    xq[s][m] = *reinterpret_cast<const bf16x8*>(&buf[xb[s % 3] + (((s / 9) * HH + m + (s / 3) % 3) * WWP) * 16]);
#pragma unroll
            for (int s = 0; s < S; s++) {
#pragma unroll
                for (int t = 0; t < NT; t++)
#pragma unroll
                    for (int m = 0; m < MT; m++)
                        acc[m][t] = RU3D_MFMA_32X32X16(wq[s % WD][t], xq[s % XD][m], acc[m][t], 0, 0, 0);
                if (s + XD < S) {
                    const int s1 = s + XD;
#pragma unroll
                    for (int m = 0; m < MT; m++)
                        xq[s % XD][m] =
                            *reinterpret_cast<const bf16x8*>(&buf[xb[s1 % 3] + (((s1 / 9) * HH + m + (s1 / 3) % 3) * WWP) * 16]);
                }
                {   // the ring never stops: the last WD steps fetch the first fragments of the next item's chunk
                    const int s2 = s + WD < S ? s + WD : s + WD - S;
                    const int c2 = s + WD < S ? ch : chn;
                    const int wtap2 = a.flip ? 26 - s2 : s2;
#pragma unroll
                    for (int t = 0; t < NT; t++) wq[s % WD][t] = wbase[((int64_t)(wtap2 * KS + c2) * NTT + t) * 64];
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            if (ch == nchunks - 1) {
                // ---- epilogue through a wave-private LDS patch (see conv3_s1_pc_kernel): bias before the transpose,
                // statistics and residual after it, 16-byte stores that cover whole 64-byte channel rows
                int n, d0, h0, w0;
                tile_origin(tile, n, d0, h0, w0);
                if (a.stat_slab && n != cur_n) {
                    stat_flush();
                    cur_n = n;
                }
                bf16* est = lds + 2 * BUF + wave * (MT * 32 * MF_PITCH);
#pragma unroll
                for (int t = 0; t < NT; t++) {
                    f32x4 bq[4];
#pragma unroll
                    for (int q = 0; q < 4; q++) bq[q] = *reinterpret_cast<const f32x4*>(&biasl[t * 32 + 8 * q + 4 * ph]);
#pragma unroll
                    for (int m = 0; m < MT; m++) {
#pragma unroll
                        for (int q = 0; q < 4; q++) {
                            float v[4];
#pragma unroll
                            for (int i = 0; i < 4; i++) v[i] = acc[m][t][q * 4 + i] + bq[q][i];
                            store_vec<bf16, 4>(est + (m * 32 + wl) * MF_PITCH + 8 * q + 4 * ph, v);
                        }
                    }
                    float st1[8], st2[8];
#pragma unroll
                    for (int i = 0; i < 8; i++) st1[i] = st2[i] = 0.f;
                    const int part = lane & 3;
#pragma unroll
                    for (int r = 0; r < 2 * MT; r++) {
                        const int row = (lane >> 2) + 16 * r;
                        const int od = d0 + wave, oh = h0 + (row >> 5), ow = w0 + (row & 31);
                        float v[8];
                        load_vec<bf16, 8>(est + row * MF_PITCH + part * 8, v);
                        if (od < a.D && oh < a.H && ow < a.W) {
                            const int64_t vox = (((int64_t)n * a.D + od) * a.H + oh) * a.W + ow;
                            const int c0 = co_blk + t * 32 + part * 8;
                            if (a.stat_slab) {
#pragma unroll
                                for (int i = 0; i < 8; i++) {
                                    st1[i] += v[i];
                                    st2[i] = fmaf(v[i], v[i], st2[i]);
                                }
                            }
                            if (a.res) {
                                float rr[8];
                                load_vec<bf16, 8>(a.res + vox * a.ldr + c0, rr);
#pragma unroll
                                for (int i = 0; i < 8; i++) v[i] += rr[i];
                            }
                            store_vec<bf16, 8>(a.y + vox * a.ldy + c0, v);
                        }
                    }
                    if (a.stat_slab) {
#pragma unroll
                        for (int i = 0; i < 8; i++) {
                            float s1 = st1[i], s2 = st2[i];
#pragma unroll
                            for (int o = 4; o < 64; o <<= 1) {   // lanes that share (lane & 3) hold the same 8 channels
                                s1 += __shfl_xor(s1, o, 64);
                                s2 += __shfl_xor(s2, o, 64);
                            }
                            if (lane < 4) {
                                const int c = t * 32 + lane * 8 + i;
                                statl[wave][c * 2] += s1;
                                statl[wave][c * 2 + 1] += s2;
                            }
                        }
                    }
                }
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    }
    stat_flush();
}


// ---------------------------------------------------------------------------------------------------------
// sk: the deep levels (16^3 x 256, 8^3 x 512 channels) with the accumulator blocking of pc4 and the reduction dimension
// split over the workgroup's four consumer waves.  The 256-voxel x 32-cout tiles of conv3_s1_mfma_kernel give a wave 1 x 2
// accumulators: 1 KB of activations from LDS and 512 B of weights through the L1 per MFMA, both pipes at their peak
// (profiles/r04_pmc_deep_levels.txt).  4 x 2 accumulators halve both, but a 128-voxel x 64-cout block per WAVE leaves only
// 64 blocks at 16^3 x 256: so all four waves of a workgroup work on the SAME 128 x 64 block, each on its own quarter of
// the input channels (private halo buffers, 16-channel chunks moved by the producer waves' LDS-DMA one chunk ahead,
// weight ring across chunks as in pc4); at the end the waves exchange accumulators through LDS - wave w keeps voxel tile
// w and receives the three other waves' partial sums for it, added in a fixed order - and each runs the epilogue of its
// 32 voxels.  gridDim.z > 1 splits the channels over workgroups as well (8^3: 4 x 4 = 16 slices of 32 channels): fp32
// partial slices in a.part, summed by the caller's next kernel or conv_ksplit_reduce_kernel.
// A wave numbers its accumulators from its own tile on (local m <-> voxel tile (m + wave) & 3): every register index is
// static.  Tile: 2 x (64 / TW) x TW voxels; a fragment's 32 voxels are 32 / TW rows of TW.
template <int TW>
__global__ __launch_bounds__(512, 2) void conv3_s1_sk_kernel(MfmaConvArgs a) {
    constexpr int TD = 2, TH = 64 / TW, R = 32 / TW, MT = 4, NT = 2, WD = 3;
    constexpr int HD = TD + 2, HH = TH + 2, WW = TW + 2;
    constexpr int SLOTS = HD * HH * WW;                  // real 32-byte voxel slots of one wave's halo
    constexpr int NCH = (SLOTS * 2 + 63) / 64;           // 1 KB DMA chunks per halo
    constexpr int BUF = NCH * 512;                       // bf16 elements per halo buffer (whole chunks)
    constexpr int S = 27, XD = 2;
    constexpr int OOBV = (int)0x80000000;
    constexpr int REDF = 4 * 3 * NT * 4 * 64 * 4;        // floats of the accumulator exchange
    static_assert(2 * 4 * BUF * 2 >= REDF * 4, "the exchange lives in the halo buffers");
    __shared__ __attribute__((aligned(1024))) bf16 lds[2 * 4 * BUF];
    __shared__ __attribute__((aligned(16))) bf16 patch[4][32 * MF_PITCH];
    __shared__ __attribute__((aligned(16))) float biasl[NT * 32];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool producer = wave >= 4;
    const int cw = wave & 3;                              // consumer index (a producer feeds consumer cw)
    const int NTT = a.Cout / 32, KS = a.Cin / 16;
    const int cgs = a.Cout / 64;
    const int bz = blockIdx.z, gz = gridDim.z;
    const int cin_wave = a.Cin / (4 * gz);                // input channels of one wave
    const int nch = cin_wave / 16;
    const int k0 = (bz * 4 + cw) * nch;                   // first 16-channel chunk of this wave

    // units in [cout group][tile] order, a contiguous run per XCD: the workgroups of an XCD share their weights
    const int unit = xcd_remap(blockIdx.x, a.nblk * cgs);
    const int cg = unit / a.nblk;
    int tile = unit % a.nblk;
    const int tw_i = tile % a.tiles_w;
    tile /= a.tiles_w;
    const int th_i = tile % a.tiles_h;
    tile /= a.tiles_h;
    const int td_i = tile % a.tiles_d;
    const int n = tile / a.tiles_d;
    const int d0 = td_i * TD, h0 = th_i * TH, w0 = tw_i * TW;

    if (producer) {
        int rel[NCH], zz[NCH];
#pragma unroll
        for (int i = 0; i < NCH; i++) {
            const int piece = i * 64 + lane;
            const int slot = piece >> 1;
            const int zw = slot % WW, zh = (slot / WW) % HH, zd = slot / (WW * HH);
            const bool valid = slot < SLOTS;
            const int part = (piece & 1) ^ ((zw >> 2) & 1);
            rel[i] = valid ? (((zd * a.H + zh) * a.W + zw) * a.ldx + part * 8) * 2 : OOBV;
            zz[i] = valid ? (zd | (zh << 8) | (zw << 16)) : -1;
        }
        const int64_t sample_elems = (int64_t)a.D * a.H * a.W * a.ldx;
        const ru3d_i32x4 rsrc = ru3d_buffer_rsrc(a.x + n * sample_elems, (int)(sample_elems * 2));
        const bool interior = d0 >= 1 && d0 + TD + 1 <= a.D && h0 >= 1 && h0 + TH + 1 <= a.H && w0 >= 1 && w0 + TW + 1 <= a.W;
        for (int it = 0; it <= nch; it++) {
            if (it < nch) {
                const int base = ((((d0 - 1) * a.H + (h0 - 1)) * a.W + (w0 - 1)) * a.ldx + (k0 + it) * 16) * 2;
                const bf16* dst = lds + ((it & 1) * 4 + cw) * BUF;
#pragma unroll
                for (int i = 0; i < NCH; i++) {
                    int off = zz[i] >= 0 ? base + rel[i] : OOBV;
                    if (!interior && zz[i] >= 0) {
                        const int gd = d0 - 1 + (zz[i] & 255), gh = h0 - 1 + ((zz[i] >> 8) & 255),
                                  gw = w0 - 1 + ((zz[i] >> 16) & 255);
                        if (!(gd >= 0 && gd < a.D && gh >= 0 && gh < a.H && gw >= 0 && gw < a.W)) off = OOBV;
                    }
                    ru3d_lds_dma16(rsrc, dst + i * 512, off);
                }
            }
            asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
        }
        return;
    }

    // ---------------------------------------------------------------------- consumer waves
    const int co_blk = cg * (NT * 32);
    const int ph = lane >> 5, wl = lane & 31;
    const int rl = wl / TW, wv = wl % TW;
    int xbm[MT][3];     // element offset (inside a buffer pair half) of this lane's piece: local tile m, W offset of the tap
#pragma unroll
    for (int m = 0; m < MT; m++) {
        const int gm = (m + wave) & 3;
#pragma unroll
        for (int tw = 0; tw < 3; tw++) {
            const int zw = wv + tw;
            xbm[m][tw] = ((((gm >> 1) * HH + (gm & 1) * R + rl) * WW) + zw) * 16 + ((ph ^ ((zw >> 2) & 1)) << 3) + wave * BUF;
        }
    }
    const bf16x8* wbase = a.w + (int64_t)cg * NT * 64 + lane;
    if (wave == 0) biasl[lane] = (a.bias && !a.part) ? a.bias[co_blk + lane] : 0.f;

    f32x16 acc[MT][NT];
#pragma unroll
    for (int m = 0; m < MT; m++)
#pragma unroll
        for (int t = 0; t < NT; t++)
#pragma unroll
            for (int i = 0; i < 16; i++) acc[m][t][i] = 0.f;
    bf16x8 wq[WD][NT];
#pragma unroll
    for (int s = 0; s < WD; s++) {
        const int wtap = a.flip ? 26 - s : s;
#pragma unroll
        for (int t = 0; t < NT; t++) wq[s][t] = wbase[((int64_t)(wtap * KS + k0) * NTT + t) * 64];
    }

    for (int it = 0; it <= nch; it++) {
        if (it >= 1) {
            const int ch = it - 1;
            const int chn = ch + 1 == nch ? ch : ch + 1;      // the last chunk's tail fetches stay inside the slice
            const bf16* buf = lds + ((ch & 1) * 4) * BUF;
            bf16x8 xq[XD][MT];
#pragma unroll
            for (int s = 0; s < XD; s++)
#pragma unroll
                for (int m = 0; m < MT; m++)
                    xq[s][m] = *reinterpret_cast<const bf16x8*>(&buf[xbm[m][s % 3] + (((s / 9) * HH + (s / 3) % 3) * WW) * 16]);
#pragma unroll
            for (int s = 0; s < S; s++) {
#pragma unroll
                for (int t = 0; t < NT; t++)
#pragma unroll
                    for (int m = 0; m < MT; m++)
                        acc[m][t] = RU3D_MFMA_32X32X16(wq[s % WD][t], xq[s % XD][m], acc[m][t], 0, 0, 0);
                if (s + XD < S) {
                    const int s1 = s + XD;
#pragma unroll
                    for (int m = 0; m < MT; m++)
                        xq[s % XD][m] =
                            *reinterpret_cast<const bf16x8*>(&buf[xbm[m][s1 % 3] + (((s1 / 9) * HH + (s1 / 3) % 3) * WW) * 16]);
                }
                {
                    const int s2 = s + WD < S ? s + WD : s + WD - S;
                    const int c2 = s + WD < S ? ch : chn;
                    const int wtap2 = a.flip ? 26 - s2 : s2;
#pragma unroll
                    for (int t = 0; t < NT; t++) wq[s % WD][t] = wbase[((int64_t)(wtap2 * KS + k0 + c2) * NTT + t) * 64];
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    }

    // ---- exchange: every halo has been read (the barrier above), the buffers now carry accumulators.
    // float4 slot [owner tile][source 0..2][t][q][lane]; a wave sends local tiles 1..3, which are tiles (m + wave) & 3
    f32x4* red = reinterpret_cast<f32x4*>(lds);
#pragma unroll
    for (int m = 1; m < MT; m++) {
        const int owner = (m + wave) & 3;
#pragma unroll
        for (int t = 0; t < NT; t++)
#pragma unroll
            for (int q = 0; q < 4; q++) {
                f32x4 v;
#pragma unroll
                for (int i = 0; i < 4; i++) v[i] = acc[m][t][q * 4 + i];
                red[(((owner * 3 + (m - 1)) * NT + t) * 4 + q) * 64 + lane] = v;
            }
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
#pragma unroll
    for (int sl = 0; sl < 3; sl++)
#pragma unroll
        for (int t = 0; t < NT; t++)
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const f32x4 v = red[(((wave * 3 + sl) * NT + t) * 4 + q) * 64 + lane];
#pragma unroll
                for (int i = 0; i < 4; i++) acc[0][t][q * 4 + i] += v[i];
            }

    // ---- epilogue of this wave's 32 voxels (tile `wave`)
    const int od_w = d0 + (wave >> 1), hrow = h0 + (wave & 1) * R;
    if (a.part) {
        const int od = od_w, oh = hrow + rl, ow = w0 + wv;
        if (od < a.D && oh < a.H && ow < a.W) {
            const int64_t vox = (((int64_t)n * a.D + od) * a.H + oh) * a.W + ow;
            float* pp = a.part + ((int64_t)bz * ((int64_t)a.N * a.D * a.H * a.W) + vox) * a.Cout;
#pragma unroll
            for (int t = 0; t < NT; t++)
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    f32x4 v;
#pragma unroll
                    for (int i = 0; i < 4; i++) v[i] = acc[0][t][q * 4 + i];
                    *reinterpret_cast<f32x4*>(pp + co_blk + t * 32 + 8 * q + 4 * ph) = v;
                }
        }
        return;
    }
    bf16* est = patch[wave];
#pragma unroll
    for (int t = 0; t < NT; t++) {
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const f32x4 bq = *reinterpret_cast<const f32x4*>(&biasl[t * 32 + 8 * q + 4 * ph]);
            float v[4];
#pragma unroll
            for (int i = 0; i < 4; i++) v[i] = acc[0][t][q * 4 + i] + bq[i];
            store_vec<bf16, 4>(est + wl * MF_PITCH + 8 * q + 4 * ph, v);
        }
        const int part = lane & 3;
#pragma unroll
        for (int r = 0; r < 2; r++) {
            const int row = (lane >> 2) + 16 * r;
            const int od = od_w, oh = hrow + row / TW, ow = w0 + row % TW;
            float v[8];
            load_vec<bf16, 8>(est + row * MF_PITCH + part * 8, v);
            if (od < a.D && oh < a.H && ow < a.W) {
                const int64_t vox = (((int64_t)n * a.D + od) * a.H + oh) * a.W + ow;
                const int c0 = co_blk + t * 32 + part * 8;
                if (a.res) {
                    float rr[8];
                    load_vec<bf16, 8>(a.res + vox * a.ldr + c0, rr);
#pragma unroll
                    for (int i = 0; i < 8; i++) v[i] += rr[i];
                }
                store_vec<bf16, 8>(a.y + vox * a.ldy + c0, v);
            }
        }
    }
}


// y = bf16(sum_z part[z] + bias) (+ residual): fixed summation order, 8 channels (16 B) per thread
__global__ __launch_bounds__(256) void conv_ksplit_reduce_kernel(const float* __restrict__ part, int ksplit, int64_t V,
                                                                 int Cout, const float* __restrict__ bias,
                                                                 const bf16* __restrict__ res, int ldr,
                                                                 bf16* __restrict__ y, int ldy) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int cg = Cout / 8;
    if (g >= V * cg) return;
    const int64_t vox = g / cg;
    const int c0 = (int)(g % cg) * 8;
    float v[8];
#pragma unroll
    for (int i = 0; i < 8; i++) v[i] = bias ? bias[c0 + i] : 0.f;
    for (int z = 0; z < ksplit; z++) {
        const float* p = part + ((int64_t)z * V + vox) * Cout + c0;
        const f32x4 lo = *reinterpret_cast<const f32x4*>(p), hi = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            v[i] += lo[i];
            v[4 + i] += hi[i];
        }
    }
    if (res) {
        float r[8];
        load_vec<bf16, 8>(res + vox * ldr + c0, r);
#pragma unroll
        for (int i = 0; i < 8; i++) v[i] = (float)(bf16)v[i] + r[i];   // same two roundings as the fused epilogues
    }
    store_vec<bf16, 8>(y + vox * ldy + c0, v);
}

// ---------------------------------------------------------------------------------------------------------
// Host side of the 3x3x3 stride-1 family: conv3_s1_plan decides, launch_s1_choice launches, conv_mfma_launch_inner (below)
// walks the plan's choices with what only the launch knows.
typedef void (*S1Kernel)(MfmaConvArgs);

static int cdiv(int x, int y) { return (x + y - 1) / y; }
static bool aligned_to(const void* p, size_t a) { return (((uintptr_t)p) % a) == 0; }
static bool s1_tilefit() {
    static const int fit_mode = ru3d_env_int("RU3D_CONV_TILEFIT", 1);
    return fit_mode != 0;
}

// Width class of the 256-voxel tiles (32: 2 x 4 x 32, 16: 2 x 8 x 16, 8: 4 x 8 x 8; the weight gradient's tiles too): W
// decides.  Extents that fit none of the tiles (config 4: 160 x 160 x 80 -> 40 x 40 x 20 on the 128-channel level) take
// the tile with the least padded volume (RU3D_CONV_TILEFIT=0: W alone).
static int s1_width_class(int D, int H, int W) {
    const int wc = W >= 24 ? 32 : (W >= 12 ? 16 : 8);
    if (!s1_tilefit()) return wc;
    auto vol = [&](int a, int b, int c) { return (int64_t)cdiv(D, a) * a * cdiv(H, b) * b * cdiv(W, c) * c; };
    const int64_t v32 = vol(2, 4, 32), v16 = vol(2, 8, 16), v8 = vol(4, 8, 8);
    const int64_t cur = wc == 32 ? v32 : (wc == 16 ? v16 : v8);
    // a narrower tile has more halo per voxel: it must save an eighth of the padded volume to be chosen
    if (wc == 32 && v16 * 8 < cur * 7 && v16 <= v8) return 16;
    if (wc >= 16 && v8 * 8 < cur * 7) return 8;
    return wc;
}
// (TD, TH) of the width class's tile with mt x 128 voxels
static void s1_tile_dims(int wc, int mt, int* td, int* th) {
    *th = wc == 32 ? 4 : 8;
    *td = (wc == 8 ? 4 : 2) * mt / 2;
}

// persistent grid of the producer/consumer kernels (and the layout of their statistics slab)
static void pc_grid(int cout, bool nt2, int64_t nblk, int* gx, int* gy) {
    *gy = cout / (nt2 ? 64 : 32);
    int g = ru3d_get_cu_budget() / *gy;   // one persistent workgroup per CU in total (N > 1: minus the CUs left to RCCL)
    g = g < 8 ? 8 : (g / 8) * 8;        // multiple of 8 so that blockIdx.x % 8 is the XCD label for every y
    if (g > nblk) g = (int)nblk;
    *gx = g;
}

static void s1_push(Conv3S1Plan& p, int family, int td, int th, int tw, int mt, int nt, int ks) {
    Conv3S1Choice& c = p.choice[p.count++];
    c.family = family; c.td = td; c.th = th; c.tw = tw; c.mt = mt; c.nt = nt; c.ks = ks;
    switch (family) {
        case S1_SLIDE32: snprintf(c.name, sizeof(c.name), "conv3_s1_slide32"); break;
        case S1_SLIDE64: snprintf(c.name, sizeof(c.name), "conv3_s1_slide64"); break;
        case S1_WS: snprintf(c.name, sizeof(c.name), "conv_ws"); break;
        case S1_PC4: snprintf(c.name, sizeof(c.name), "conv3_s1_pc4"); break;
        case S1_SK: snprintf(c.name, sizeof(c.name), "conv3_s1_sk<%d>", tw); break;
        default:
            snprintf(c.name, sizeof(c.name), "%s<%d,%d,%d,%d,%d>", family == S1_PC ? "conv3_s1_pc" : "conv3_s1_mfma", td, th,
                     tw, mt, nt);
    }
}

Conv3S1Plan conv3_s1_plan(const ConvGeom& g) {
    // the family's switches, each read once per process; 0 = that kernel off
    static const int slide_mode = ru3d_env_int("RU3D_CONV_SLIDE", 1), slide64_mode = ru3d_env_int("RU3D_CONV_SLIDE64", 1);
    static const int edge_mode = ru3d_env_int("RU3D_SLIDE64_EDGE", 1);
    static const int ws_mode = ru3d_env_int("RU3D_CONV_WS", 1);       // 2: wherever the shape fits
    static const int pc_mode = ru3d_env_int("RU3D_CONV_PC", 1), pc4_mode = ru3d_env_int("RU3D_CONV_PC4", 1);
    static const int sk_mode = ru3d_env_int("RU3D_CONV_SK", 1);       // 2: also where under 30 % of the MFMAs are useful
    Conv3S1Plan p;
    if (!(g.k == 3 && g.stride == 1 && !g.transposed && (g.Cin % 32) == 0 && (g.Cout % 32) == 0)) return p;
    const int N = g.N, D = g.Do, H = g.Ho, W = g.Wo, Cin = g.Cin, Cout = g.Cout, ldx = g.ldx;
    const bool buffer_ok = ldx > 0 && (ldx % 8) == 0 && (int64_t)D * H * W * ldx * 2 < (1ll << 31);   // a sample a descriptor can address

    // 1. the large levels with 32 / 64 input channels: the D-sliding kernels
    if (slide_mode && slide_conv_plan(N, D, H, W, Cin, Cout, &p.slide)) s1_push(p, S1_SLIDE32, 0, 0, 0, 0, 0, 1);
    else if (slide64_mode && slide64_conv_plan(N, D, H, W, Cin, Cout, edge_mode != 0, &p.slide)) s1_push(p, S1_SLIDE64, 0, 0, 0, 0, 0, 1);
    const bool slide = p.count > 0;
    // 2. the deepest level: whole-sample workgroups that read their weight slice once (conv_ws.hip), then the split-K sum
    if (const int wsl = ws_mode ? conv_ws_slices(N, D, H, W, Cin, Cout, ws_mode) : 0) s1_push(p, S1_WS, 0, 0, 0, 0, 0, wsl);

    // 3. tiles.  W decides the tile's aspect; if the 256-voxel x 64-cout decomposition yields fewer than ~2 workgroups per
    // CU (deep levels: 16^3, 8^3) the 64-cout slices go; >= 2 (tile, cout-slice) units per CU run on the persistent
    // producer/consumer kernel
    const int wc = s1_width_class(D, H, W);
    int td, th;
    s1_tile_dims(wc, 2, &td, &th);
    int64_t nblk_pc = (int64_t)N * cdiv(D, td) * cdiv(H, th) * cdiv(W, wc);     // spatial tiles of the pc decomposition
    const bool can_nt2 = (Cout % 64) == 0;
    const bool small = nblk_pc * (Cout / (can_nt2 ? 64 : 32)) < 512;
    const bool nt2 = can_nt2 && !small;
    const bool pc = !small && pc_mode >= 1 && (wc >= 16 || s1_tilefit());
    if (!small) {
        // the 512-voxel form: no more padded volume than the 2 x 4 x 32 tile, at least 3/4 of the CUs busy
        const int64_t n4 = (int64_t)N * (D / 4) * (H / 4) * cdiv(W, 32);
        if (pc && nt2 && wc == 32 && pc4_mode && (D % 4) == 0 && (H % 4) == 0 && buffer_ok &&
            n4 * (Cout / 64) * 4 >= (int64_t)ru3d_get_cu_budget() * 3) {
            nblk_pc = n4;
            s1_push(p, S1_PC4, 4, 4, 32, 2, 2, 1);
        } else {
            s1_push(p, pc ? S1_PC : S1_TILE, td, th, wc, 2, nt2 ? 2 : 1, 1);
        }
    } else {
        // deep levels: 128-voxel x 64-cout blocks with the input channels split over the workgroup's waves and, below
        // 192 blocks, over workgroups (conv3_s1_sk_kernel).  Tile width with the smaller padded volume (ties: the wider
        // one); ragged extents are masked in the kernel
        const int64_t v16 = (int64_t)cdiv(D, 2) * 2 * cdiv(H, 4) * 4 * cdiv(W, 16) * 16;
        const int64_t v8 = (int64_t)cdiv(D, 2) * 2 * cdiv(H, 8) * 8 * cdiv(W, 8) * 8;
        const int tw = v16 <= v8 ? 16 : 8;
        const int64_t sk_units = (int64_t)N * cdiv(D, 2) * cdiv(H, 64 / tw) * cdiv(W, tw) * (Cout / 64);
        if (sk_mode && can_nt2 && (Cin % 64) == 0 && buffer_ok && sk_units <= 512 &&
            (sk_mode >= 2 || (int64_t)D * H * W * 10 >= (tw == 16 ? v16 : v8) * 3)) {
            int ks = 1;
            while (sk_units * ks < 192 && ks < 8 && ((Cin / (ks * 2)) % 64) == 0) ks *= 2;
            if (sk_units * ks >= 96) s1_push(p, S1_SK, 2, 64 / tw, tw, 0, 0, ks);
        }
        // then 256-voxel tiles x 32-cout slices: the deep levels are bound by the weight bytes every workgroup pulls into
        // its CU, which these halve against the 128-voxel tiles.  One workgroup per CU is the aim: fewer (8^3) split the
        // 32-channel chunks over gridDim.z (fp32 partials in the caller's scratch).  Splitting further, to two resident
        // workgroups per CU, measured slower in round 3 (16^3: 38.8 -> 43.1 us, 8^3: 26.8 -> 28.2 us)
        const int64_t units = nblk_pc * (Cout / 32);
        int ks = 1;
        if (units < 256 && Cin >= 64)
            for (ks = 2; ks * 2 <= Cin / 32 && units * ks < 256;) ks *= 2;
        if (ks > 1 || units >= 256) s1_push(p, S1_TILE, td, th, wc, 2, 1, ks);
        // ... and where that needs scratch the caller did not pass, or one chunk is all there is: 128-voxel tiles
        if (ks > 1 || units < 256) {
            s1_tile_dims(wc, 1, &td, &th);
            s1_push(p, S1_TILE, td, th, wc, 1, 1, 1);
        }
    }

    pc_grid(Cout, nt2, nblk_pc, &p.pc_gx, &p.pc_gy);
    // split-K scratch: none when a sliding kernel is the first choice, the whole-sample kernel's when it is; else the most
    // any choice can use
    const size_t slice = (size_t)N * D * H * W * Cout * sizeof(float);
    for (int i = 0; i < p.count && !slide; i++) {
        const Conv3S1Choice& c = p.choice[i];
        if (c.family == S1_WS) {
            p.ws_bytes = c.ks * slice;
            break;
        }
        if (c.ks > 1 && c.ks * slice > p.ws_bytes) p.ws_bytes = c.ks * slice;
    }
    // fused forms: the statistics slab follows the grid of the kernel that fills it
    p.can_bwd_sums = p.can_partner = slide && p.choice[0].family == S1_SLIDE32;
    p.can_stats = slide || pc;
    if (slide) {
        p.gx = p.slide.grid;
        p.gy = p.slide.ny;
        p.cb = (p.choice[0].family == S1_SLIDE32 || Cout == 32) ? 32 : 64;
    } else {
        p.gx = p.pc_gx;
        p.gy = p.pc_gy;
        p.cb = nt2 ? 64 : 32;
    }
    p.slab_bytes = (size_t)p.gx * p.gy * 4 * N * p.cb * 2 * sizeof(float);
    return p;
}

template <int TD, int TH, int TW, int MT> static S1Kernel s1_tile_kernel(int nt) {
    return nt == 2 ? conv3_s1_mfma_kernel<TD, TH, TW, MT, 2> : conv3_s1_mfma_kernel<TD, TH, TW, MT, 1>;
}
template <int TD, int TH, int TW> static S1Kernel s1_pc_kernel(int nt) {
    return nt == 2 ? conv3_s1_pc_kernel<TD, TH, TW, 2, 2> : conv3_s1_pc_kernel<TD, TH, TW, 2, 1>;
}
// the one (family, tile, mt, nt) -> instantiation ladder
static S1Kernel s1_kernel(const Conv3S1Choice& c) {
    switch (c.family) {
        case S1_PC4: return conv3_s1_pc4_kernel<3>;
        case S1_SK: return c.tw == 16 ? conv3_s1_sk_kernel<16> : conv3_s1_sk_kernel<8>;
        case S1_PC:
            return c.tw == 32 ? s1_pc_kernel<2, 4, 32>(c.nt) : c.tw == 16 ? s1_pc_kernel<2, 8, 16>(c.nt) : s1_pc_kernel<4, 8, 8>(c.nt);
        default:
            if (c.mt == 2)
                return c.tw == 32 ? s1_tile_kernel<2, 4, 32, 2>(c.nt)
                                  : c.tw == 16 ? s1_tile_kernel<2, 8, 16, 2>(c.nt) : s1_tile_kernel<4, 8, 8, 2>(c.nt);
            return c.tw == 32 ? s1_tile_kernel<1, 4, 32, 1>(c.nt)
                              : c.tw == 16 ? s1_tile_kernel<1, 8, 16, 1>(c.nt) : s1_tile_kernel<2, 8, 8, 1>(c.nt);
    }
}

// the caller's scratch holds ks slices of partials, and y / res take the 16-byte rows of the sum that follows
static bool s1_scratch_ok(const MfmaConvArgs& a, int ks) {
    const size_t bytes = (size_t)ks * a.N * a.D * a.H * a.W * a.Cout * sizeof(float);
    return a.ws && a.ws_bytes >= bytes && aligned_to(a.ws, 16) && (a.ldy % 8) == 0 && (!a.res || (a.ldr % 8) == 0);
}

// ks slices of fp32 partials in a.ws -> y: the caller's next kernel sums them (defer_ks: norm_small.hip), or the
// fixed-order reduce here, with the bias / residual fused
static int s1_splitk_tail(const MfmaConvArgs& a, int ks, hipStream_t st) {
    if (a.defer_ks) {
        *a.defer_ks = ks;
        return 0;
    }
    const int64_t V = (int64_t)a.N * a.D * a.H * a.W;
    const int64_t groups = V * (a.Cout / 8);
    hipLaunchKernelGGL(conv_ksplit_reduce_kernel, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, st,
                       (const float*)a.ws, ks, V, a.Cout, a.bias, a.res, a.ldr, a.y, a.ldy);
    return ru3d_check_launch("conv_ksplit_reduce");
}

static int launch_s1_choice(const MfmaConvArgs& a0, const Conv3S1Plan& p, const Conv3S1Choice& c, hipStream_t st) {
    MfmaConvArgs a = a0;
    if (c.family == S1_WS) {
        if (int rc = conv_ws_launch(a.x, a.w, (float*)a.ws, a.N, a.D, a.H, a.W, a.Cin, a.Cout, a.ldx, a.flip, c.ks, st)) return rc;
        return s1_splitk_tail(a, c.ks, st);
    }
    a.tiles_d = cdiv(a.D, c.td);
    a.tiles_h = cdiv(a.H, c.th);
    a.tiles_w = cdiv(a.W, c.tw);
    const int64_t nblk = (int64_t)a.N * a.tiles_d * a.tiles_h * a.tiles_w;
    if (nblk > 0x7fffffff) return ru3d_fail(-1, "conv_mfma: grid too large");
    a.nblk = (int)nblk;
    a.ksplit = c.ks;
    a.part = c.ks > 1 ? (float*)a.ws : nullptr;
    dim3 grid(p.pc_gx, p.pc_gy), block(512);      // the persistent kernels
    if (c.family == S1_SK) grid = dim3((unsigned)(nblk * (a.Cout / 64)), 1, c.ks);
    if (c.family == S1_TILE) {
        grid = dim3((unsigned)nblk, a.Cout / (32 * c.nt), c.ks);
        block = dim3(256);
    }
    hipLaunchKernelGGL(s1_kernel(c), grid, block, 0, st, a);
    const int rc = ru3d_check_launch(c.name);
    return (rc || c.ks <= 1) ? rc : s1_splitk_tail(a, c.ks, st);
}

// mean / scale from the slabs: one thread block per (n, 4 channels); 64 lanes per channel sum the
// (workgroup, wave) partials in a fixed order, in double.
__global__ __launch_bounds__(256) void stats_slab_finalize_kernel(const float* __restrict__ slab, int gx, int cb, int N,
                                                                  int C, double invV, const float* __restrict__ drop,
                                                                  float eps, float* __restrict__ mean,
                                                                  float* __restrict__ scale) {
    const int lane = threadIdx.x & 63, cx = threadIdx.x >> 6;
    const int n = blockIdx.y, c = blockIdx.x * 4 + cx;
    double a1 = 0.0, a2 = 0.0;
    if (c < C) {
        const int y = c / cb, cl = c % cb;
        const int parts = gx * 4;   // (workgroup x, wave) pairs that hold channel c
        // the lane's chain over p = lane, lane + 64, ... ascending, SLAB_BATCH pairs loaded before the first add (one
        // round trip for up to 256 workgroups per row, where every pair used to wait for the one before); a pair past
        // the end is loaded from the batch's first and not added
        constexpr int SLAB_BATCH = 16;
        for (int p0 = lane; p0 < parts; p0 += 64 * SLAB_BATCH) {
            float e0[SLAB_BATCH], e1[SLAB_BATCH];
#pragma unroll
            for (int j = 0; j < SLAB_BATCH; j++) {
                const int p = p0 + 64 * j < parts ? p0 + 64 * j : p0;
                const float* e = slab + ((((int64_t)(y * gx + (p >> 2)) * 4 + (p & 3)) * N + n) * cb + cl) * 2;
                e0[j] = e[0];
                e1[j] = e[1];
            }
            __builtin_amdgcn_sched_barrier(0);      // or the scheduler pairs every load with its add to save registers
#pragma unroll
            for (int j = 0; j < SLAB_BATCH; j++) {
                if (p0 + 64 * j < parts) {
                    a1 += (double)e0[j];
                    a2 += (double)e1[j];
                }
            }
        }
    }
    const double t1 = wave_sum_d(a1), t2 = wave_sum_d(a2);   // xor-butterfly: fixed order
    if (lane == 0 && c < C) {
        const int i = n * C + c;
        if (!scale) {            // backward sums: mean[] receives m12 = (mean g', mean g' xhat)
            mean[2 * i] = (float)(t1 * invV);
            mean[2 * i + 1] = (float)(t2 * invV);
            return;
        }
        const double m = t1 * invV;
        double var = t2 * invV - m * m;
        if (var < 0.0) var = 0.0;
        const double sdrop = drop ? (double)drop[i] : 1.0;
        mean[i] = (float)m;
        scale[i] = (float)(sdrop / sqrt(sdrop * sdrop * var + (double)eps));
    }
}

int stats_slab_finalize_launch(const float* slab, int gx, int cb, int N, int C, double invV, const float* drop, float eps,
                               float* mean, float* scale, hipStream_t st) {
    dim3 grid((C + 3) / 4, N);
    hipLaunchKernelGGL(stats_slab_finalize_kernel, grid, dim3(256), 0, st, slab, gx, cb, N, C, invV, drop, eps, mean, scale);
    return ru3d_check_launch(scale ? "stats_slab_finalize" : "bwd_sums_slab_finalize");
}

// Every data-movement form with MFMA-friendly channel counts runs on MFMA: the 3x3x3 stride-1 gather with
// Cin % 32 == 0 on the LDS-halo kernel, everything else on the direct family (conv_direct.hip, same packed-weight layout).
bool mfma_conv_geometry_ok(const ConvGeom& g) { return !g.transposed || g.stride == 2; }

static int conv_mfma_launch_inner(const void* x, const void* w, const float* bias, const void* res, void* y,
                                  const ConvGeom& g, const Conv3S1Plan& p, hipStream_t st, float* stat_slab, void* ws,
                                  size_t ws_bytes, const void* bst_act, int bst_ld, float slope, const void* x2, int ldx2,
                                  const void* w2, int* defer_ks);

int conv_mfma_launch(const void* x, const void* w, const float* bias, const void* res, void* y, const ConvGeom& g,
                     hipStream_t st, float* stat_slab, void* ws, size_t ws_bytes, const void* bst_act, int bst_ld,
                     float slope, const void* x2, int ldx2, const void* w2, int* defer_ks, const Conv3S1Plan* plan) {
    // bench.py's kernel probe: an event pair around the conv kernel itself (ru3d_probe_begin; comm.hip)
    void* stop = (g.k == 3 && g.stride == 1 && !g.transposed)
                     ? ru3d_probe_start(g.N, g.Do, g.Ho, g.Wo, g.Cin, g.Cout, st) : nullptr;
    const int rc = conv_mfma_launch_inner(x, w, bias, res, y, g, plan ? *plan : conv3_s1_plan(g), st, stat_slab, ws, ws_bytes,
                                          bst_act, bst_ld, slope, x2, ldx2, w2, defer_ks);
    ru3d_probe_stop(stop, st);
    return rc;
}

static int conv_mfma_launch_inner(const void* x, const void* w, const float* bias, const void* res, void* y,
                                  const ConvGeom& g, const Conv3S1Plan& p, hipStream_t st, float* stat_slab, void* ws,
                                  size_t ws_bytes, const void* bst_act, int bst_ld, float slope, const void* x2, int ldx2,
                                  const void* w2, int* defer_ks) {
    if (defer_ks) *defer_ks = 0;
    if (!mfma_conv_geometry_ok(g)) return ru3d_fail(-1, "conv_mfma: geometry not supported");
    const int first = p.count ? p.choice[0].family : 0;
    if (g.x_cseg || g.y_cseg) {
        // planar concat (see ru3d_tensor): the decoder block's conv1 on the 64-channel sliding kernel (split input), its
        // input gradient pair on the 32-channel sliding kernel (split output: one plane per 32-channel slice)
        const bool in_ok = g.x_cseg && !g.y_cseg && first == S1_SLIDE64;
        const bool out_ok = g.y_cseg && !g.x_cseg && x2 && p.can_partner;
        if (!in_ok && !out_ok) return ru3d_fail(-1, "conv_mfma: no kernel takes this split tensor");
    }
    if (x2 && !p.can_partner) return ru3d_fail(-1, "conv_mfma: no fused 1x1 partner for this shape");
    if ((g.ldx % 8) || (g.ldy % 4) || (res && (g.ldr % 4)) || !aligned_to(x, 16) || !aligned_to(y, 8) ||
        (res && !aligned_to(res, 8)) || (bias && !aligned_to(bias, 16)) || !aligned_to(w, 16))
        return ru3d_fail(-1, "conv_mfma: operands must be 16-byte (x, w, bias) / 8-byte (y, res) aligned");
    if (bst_act && !p.can_bwd_sums)
        return ru3d_fail(-1, "conv_mfma: fused backward sums are not available for this shape");
    if (!p.count) {
        if (stat_slab) return ru3d_fail(-1, "conv_mfma: fused statistics not available for this form");
        return conv_direct_launch(conv_direct_plan(g), x, w, bias, res, y, g, st);
    }
    MfmaConvArgs a;
    a.x = (const bf16*)x;
    a.w = (const bf16x8*)w;
    a.bias = bias;
    a.res = (const bf16*)res;
    a.y = (bf16*)y;
    a.N = g.N; a.D = g.Do; a.H = g.Ho; a.W = g.Wo;
    a.Cin = g.Cin; a.Cout = g.Cout; a.ldx = g.ldx; a.ldy = g.ldy; a.ldr = g.ldr;
    a.flip = g.flip;
    a.stat_slab = stat_slab;
    a.part = nullptr;
    a.ksplit = 1;
    a.defer_ks = (res || stat_slab) ? nullptr : defer_ks;
    a.ws = ws;
    a.ws_bytes = ws_bytes;
    // The first choice whose launch-time conditions hold runs; the last one has none.
    for (int i = 0; i < p.count; i++) {
        const Conv3S1Choice& c = p.choice[i];
        if (c.family == S1_SLIDE32 || c.family == S1_SLIDE64) {
            // 16-byte stores; a sample within the 30-bit element range of the staging loads' buffer offsets
            const bool aligned = (g.ldy % 8) == 0 && (!res || (g.ldr % 8) == 0) && aligned_to(y, 16) &&
                                 (!res || aligned_to(res, 16)) && (g.ldx % 8) == 0 && aligned_to(x, 16) &&
                                 (int64_t)g.Do * g.Ho * g.Wo * g.ldx < (1ll << 30) &&
                                 (!bst_act || ((bst_ld % 8) == 0 && aligned_to(bst_act, 16)));
            if (aligned)
                return c.family == S1_SLIDE32
                           ? conv_slide_launch(x, w, bias, res, y, g, p.slide, stat_slab, st, bst_act, bst_ld, slope, x2, ldx2, w2)
                           : conv_slide64_launch(x, w, bias, res, y, g, p.slide, stat_slab, st);
            if (bst_act) return ru3d_fail(-1, "conv_mfma: the fused backward sums need 16-byte aligned operands");
            if (x2) return ru3d_fail(-1, "conv_mfma: the fused 1x1 partner needs 16-byte aligned operands");
            // the statistics slab (size, layout) was planned for the sliding kernel's grid: falling back to the
            // producer/consumer kernel here would fill it with another geometry
            if (stat_slab)
                return ru3d_fail(-1, "conv_mfma: fused statistics need y (and res) 16-byte aligned with a pitch that is "
                                     "a multiple of 8 on this shape");
            continue;
        }
        if (c.family == S1_WS) {
            if (stat_slab || !s1_scratch_ok(a, c.ks)) continue;
        } else if (c.family == S1_SK || c.family == S1_TILE) {
            if (stat_slab) return ru3d_fail(-1, "conv_mfma: fused statistics need the producer/consumer kernel");
            if (c.ks > 1 && !s1_scratch_ok(a, c.ks)) continue;
        }
        return launch_s1_choice(a, p, c, st);
    }
    return ru3d_fail(-1, "conv_mfma: the plan has no choice for this launch");
}

// ---------------------------------------------------------------------------------------------------------
// Weight gradient of the 3x3x3 stride-1 conv on MFMA:
//     dW[tap][ci][co] = sum_pos X[pos + tap][ci] * DY[pos][co]
// is 27 GEMMs (M = ci, N = co, K = positions) that share the DY operand.  Both operands are K-major in
// memory (NDHWC: a position's channels are contiguous, MFMA wants 8 consecutive K per lane), so tiles are
// staged row-per-position in LDS (64-byte rows, no padding: conflict-free for the transposed read) and the
// fragments are fetched with ds_read_b64_tr_b16 (hardware 4x16 transpose).
// Workgroup = one (32 ci) x (32 co) pair; its 4 waves split the 27 taps (7/7/7/6), each wave keeping its
// taps' 32x32 fp32 accumulators in registers while the workgroup walks position tiles (persistent, stride
// G).  Partial sums go to a slab per workgroup and are reduced in fixed order (deterministic, no atomics).
struct MfmaWgradArgs {
    const bf16* x;
    const bf16* dy;
    float* part;
    int N, D, H, W;
    int Cin, Cout, ldx, lddy;
    int tiles_d, tiles_h, tiles_w, ntiles;
    int G;   // workgroups per channel pair (= number of partial slabs)
    float* dw;   // G == 1 on the deepest level: the gradient itself, [co][ci][27] (no slab, no reduce pass)
};

typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;

__device__ __forceinline__ bf16x8 tr_frag(const bf16* p) {
    // 8 consecutive K (positions) of this lane's channel: two 4-row transposed reads
    const bf16x4 lo = RU3D_DS_READ_TR16(p);
    const bf16x4 hi = RU3D_DS_READ_TR16(p + 4 * 32);
    bf16x8 r = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return r;
}

template <int TD, int TH, int TW>
__global__ __launch_bounds__(256, 2) void wgrad3_s1_mfma_kernel(MfmaWgradArgs a) {
    constexpr int HD = TD + 2, HH = TH + 2, WW = TW + 2;
    constexpr int HV = HD * HH * WW;
    static_assert(TD * TH * TW == 256, "tile must hold 256 positions");
    static_assert((HV + 256) * 64 <= 80 * 1024, "two workgroups per CU");
    __shared__ __attribute__((aligned(16))) bf16 lds[(HV + 256) * 32];
    bf16* xs = lds;             // [HV][32]  halo tile of 32 input channels
    bf16* ds = lds + HV * 32;   // [256][32] dy tile of 32 output channels

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int COT = a.Cout / 32;
    const int cit = blockIdx.y / COT, cot = blockIdx.y % COT;

    // this wave's taps: wave, wave + 4, ... (tap 27 = none)
    int toff[7];
#pragma unroll
    for (int t = 0; t < 7; t++) {
        const int tap = wave + 4 * t < 27 ? wave + 4 * t : 26;
        const int kd = tap / 9, kh = (tap / 3) % 3, kw = tap % 3;
        toff[t] = ((kd * HH + kh) * WW + kw) * 32;
    }
    f32x16 acc[7];
#pragma unroll
    for (int t = 0; t < 7; t++)
#pragma unroll
        for (int i = 0; i < 16; i++) acc[t][i] = 0.f;

    const int h = lane >> 5, cg = (lane >> 4) & 1, q = (lane & 15) >> 2, p4 = lane & 3;
    const int lane_off = q * 32 + 16 * cg + 4 * p4;   // row q of the 4x16 block, columns 4p..4p+3

    // The NEXT tile's global loads are issued before the MFMA loop of the current one and written to LDS after it:
    // the staging registers are the second buffer, the load latency hides under 112 MFMAs per wave.
    constexpr int NIT = (HV * 4 + 255) / 256;
    bf16x8 sx[NIT], sd[4];
    auto load_tile = [&](int tile) {
        int tt = tile;
        const int w0 = (tt % a.tiles_w) * TW;
        tt /= a.tiles_w;
        const int h0 = (tt % a.tiles_h) * TH;
        tt /= a.tiles_h;
        const int d0 = (tt % a.tiles_d) * TD;
        const int n = tt / a.tiles_d;
#pragma unroll
        for (int i = 0; i < NIT; i++) {
            const int c = tid + i * 256;
            const int hv = c >> 2, part = c & 3;
            const int zw = hv % WW, zh = (hv / WW) % HH, zd = hv / (WW * HH);
            const int gd = d0 + zd - 1, gh = h0 + zh - 1, gw = w0 + zw - 1;
            bf16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
            if (c < HV * 4 && gd >= 0 && gd < a.D && gh >= 0 && gh < a.H && gw >= 0 && gw < a.W)
                v = *reinterpret_cast<const bf16x8*>(a.x + ((((int64_t)n * a.D + gd) * a.H + gh) * a.W + gw) * a.ldx +
                                                     cit * 32 + part * 8);
            sx[i] = v;
        }
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int c = tid + i * 256;
            const int f = c >> 2, part = c & 3;
            const int gd = d0 + f / (TH * TW), gh = h0 + (f / TW) % TH, gw = w0 + f % TW;
            bf16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
            if (gd < a.D && gh < a.H && gw < a.W)
                v = *reinterpret_cast<const bf16x8*>(a.dy + ((((int64_t)n * a.D + gd) * a.H + gh) * a.W + gw) * a.lddy +
                                                     cot * 32 + part * 8);
            sd[i] = v;
        }
    };
    auto store_tile = [&]() {
#pragma unroll
        for (int i = 0; i < NIT; i++) {
            const int c = tid + i * 256;
            if (c < HV * 4) *reinterpret_cast<bf16x8*>(&xs[(c >> 2) * 32 + (c & 3) * 8]) = sx[i];
        }
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int c = tid + i * 256;
            *reinterpret_cast<bf16x8*>(&ds[(c >> 2) * 32 + (c & 3) * 8]) = sd[i];
        }
    };
    if ((int)blockIdx.x < a.ntiles) {
        load_tile(blockIdx.x);
        store_tile();
    }
    for (int tile = blockIdx.x; tile < a.ntiles; tile += a.G) {
        __syncthreads();   // this tile's rows are in LDS
        const bool more = tile + a.G < a.ntiles;
        if (more) load_tile(tile + a.G);
#pragma unroll
        for (int ks = 0; ks < 16; ks++) {
            // first position of this lane's 8-position half of the k-step: f0 = 16 ks + 8 h
            int hvb, f0;
            if (TW >= 16) {
                constexpr int dummy = 0;
                (void)dummy;
                const int fb = ks * 16;
                hvb = ((fb / (TH * TW)) * HH + (fb / TW) % TH) * WW + fb % TW + 8 * h;
                f0 = fb + 8 * h;
            } else {
                const int fb = ks * 16;   // two rows of 8: row 2ks (h = 0) and 2ks + 1 (h = 1), same d-plane
                hvb = ((fb / (TH * TW)) * HH + (fb / TW) % TH) * WW + h * WW;
                f0 = fb + 8 * h;
            }
            const bf16x8 bfrag = tr_frag(ds + f0 * 32 + lane_off);
#pragma unroll
            for (int t = 0; t < 7; t++) {   // tap 27 (wave 3, t = 6) recomputes tap 26 and is dropped: no branches here
                const bf16x8 afrag = tr_frag(xs + hvb * 32 + toff[t] + lane_off);
                acc[t] = RU3D_MFMA_32X32X16(afrag, bfrag, acc[t], 0, 0, 0);
            }
        }
        __syncthreads();   // every wave is done with this tile's rows
        if (more) store_tile();
    }
    if (a.dw) {
        // One workgroup holds the pair's whole sum (G == 1: 512 -> 512 on 8^3 has 256 pairs = one workgroup per CU):
        // the 32 x 32 x 27 block goes out in the parameter's own layout dw[co][ci][tap] - per output channel one run
        // of 32 * 27 floats - transposed through LDS in four quarters of 8 output channels (row pitch 868 floats:
        // 16-byte aligned rows, the 8 channel lanes on distinct banks), 16-byte coalesced stores.  No slab, no
        // reduce pass (was 26 + 18 us per layer).
        constexpr int RP = 868;
        static_assert(8 * RP * 4 <= (HV + 256) * 64, "quarter block fits the tile buffer");
        float* const fl = reinterpret_cast<float*>(lds);
        const int co_l = lane & 7, qd_mine = (lane & 31) >> 3;
        for (int qd = 0; qd < 4; qd++) {
            __syncthreads();   // the tile rows (first quarter) / the previous quarter have been read
            if (qd_mine == qd) {
#pragma unroll
                for (int t = 0; t < 7; t++) {
                    const int tap = wave + 4 * t;
                    if (tap < 27) {
#pragma unroll
                        for (int i = 0; i < 16; i++) {
                            const int ci_l = (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5);
                            fl[co_l * RP + ci_l * 27 + tap] = acc[t][i];
                        }
                    }
                }
            }
            __syncthreads();
            for (int j = tid; j < 8 * 216; j += 256) {
                const int c = j / 216, r = j - c * 216;
                const f32x4 v = *reinterpret_cast<const f32x4*>(fl + c * RP + r * 4);
                *reinterpret_cast<f32x4*>(a.dw + ((int64_t)(cot * 32 + qd * 8 + c) * a.Cin + cit * 32) * 27 + r * 4) = v;
            }
        }
        return;
    }
    // partial slab: part[((chunk * 27 + tap) * Cin + ci) * Cout + co]; D row = ci, col = co
#pragma unroll
    for (int t = 0; t < 7; t++) {
        const int tap = wave + 4 * t;
        if (tap < 27) {
            float* pp = a.part + ((int64_t)blockIdx.x * 27 + tap) * a.Cin * a.Cout;
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const int ci = cit * 32 + (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5);
                const int co = cot * 32 + (lane & 31);
                pp[(int64_t)ci * a.Cout + co] = acc[t][i];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// Weight gradient for the remaining forms (1x1x1 stride 1/2; 3x3x3 stride 2 = pooling conv and ConvTranspose):
// the gathered operand X[s*pos + tap - p] has no compact halo, so each tap's [positions][32 ci] tile is staged
// separately (row-per-position, transposed reads as above).
//   TAPS == 27: tile = 32 flat positions, all 27 tap tiles resident (55 KB); waves split the taps.
//   TAPS == 1 : tile = 256 flat positions; waves split the K (position) range and write one slab each.
struct StagedWgradArgs {
    const bf16* x;
    const bf16* dy;
    float* part;
    int N, Di, Hi, Wi, Do, Ho, Wo;
    int Cin, Cout, ldx, lddy;
    int stride, pad;
    int64_t P;       // N*Do*Ho*Wo
    int ntiles, G;
    int x_cseg;            // split x (planar concat): ci tile t lives in plane t * 32 / x_cseg
    int64_t x_segstride;
};

template <int TAPS, int PT>
__global__ __launch_bounds__(256, 2) void wgrad_staged_mfma_kernel(StagedWgradArgs a) {
    constexpr int K = (TAPS == 27) ? 3 : 1;
    __shared__ __attribute__((aligned(16))) bf16 lds[(TAPS * PT + PT) * 32];
    bf16* xs = lds;                    // [TAPS][PT][32]
    bf16* ds = lds + TAPS * PT * 32;   // [PT][32]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int COT = a.Cout / 32;
    const int cit = blockIdx.y / COT, cot = blockIdx.y % COT;
    constexpr int NACC = (TAPS == 27) ? 7 : 1;
    f32x16 acc[NACC];
#pragma unroll
    for (int t = 0; t < NACC; t++)
#pragma unroll
        for (int i = 0; i < 16; i++) acc[t][i] = 0.f;
    const int h = lane >> 5, cg = (lane >> 4) & 1, q = (lane & 15) >> 2, p4 = lane & 3;
    const int lane_off = q * 32 + 16 * cg + 4 * p4;
    const int part = tid & 3;
    const bf16* const xbase = a.x_cseg ? a.x + (int64_t)((cit * 32) / a.x_cseg) * a.x_segstride : a.x;
    const int xc0 = a.x_cseg ? (cit * 32) % a.x_cseg : cit * 32;

    for (int tile = blockIdx.x; tile < a.ntiles; tile += a.G) {
        const int64_t p_base = (int64_t)tile * PT;
        __syncthreads();
        // each thread stages a fixed 16-byte piece column (part) of fixed positions for every tap it owns
        constexpr int POS_PER_THREAD = (PT * 4 + 255) / 256;      // 4 for PT = 256, 1 for PT = 32
#pragma unroll
        for (int j = 0; j < POS_PER_THREAD; j++) {
            const int pl = ((tid >> 2) + 64 * j) % PT;
            const int64_t pos = p_base + pl;
            const bool pv = pos < a.P;
            const int64_t pp = pv ? pos : 0;
            const int ow = (int)(pp % a.Wo);
            int64_t t = pp / a.Wo;
            const int oh = (int)(t % a.Ho);
            t /= a.Ho;
            const int od = (int)(t % a.Do);
            const int n = (int)(t / a.Do);
            // dy piece (only the threads of the first 4*PT ids, i.e. every (pos, part) once)
            if (TAPS == 1 || tid < PT * 4) {
                bf16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
                if (pv) v = *reinterpret_cast<const bf16x8*>(a.dy + pos * a.lddy + cot * 32 + part * 8);
                *reinterpret_cast<bf16x8*>(&ds[pl * 32 + part * 8]) = v;
            }
            // taps owned by this thread: TAPS == 27 -> (tid >> 7) + 2 i ; TAPS == 1 -> tap 0.
            // All gathers are issued first (registers), the LDS writes follow: one exposed latency per tile.
            constexpr int TAP_ITERS = (TAPS == 27) ? 14 : 1;
            bf16x8 sx[TAP_ITERS];
#pragma unroll
            for (int i = 0; i < TAP_ITERS; i++) {
                const int tap = (TAPS == 27) ? ((tid >> 7) + 2 * i) : 0;
                const int kd = tap / (K * K), kh = (tap / K) % K, kw = tap % K;
                const int id = od * a.stride + kd - a.pad, ih = oh * a.stride + kh - a.pad,
                          iw = ow * a.stride + kw - a.pad;
                bf16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
                if (tap < TAPS && pv && id >= 0 && id < a.Di && ih >= 0 && ih < a.Hi && iw >= 0 && iw < a.Wi)
                    v = *reinterpret_cast<const bf16x8*>(xbase + ((((int64_t)n * a.Di + id) * a.Hi + ih) * a.Wi + iw) * a.ldx +
                                                         xc0 + part * 8);
                sx[i] = v;
            }
#pragma unroll
            for (int i = 0; i < TAP_ITERS; i++) {
                const int tap = (TAPS == 27) ? ((tid >> 7) + 2 * i) : 0;
                if (tap < TAPS) *reinterpret_cast<bf16x8*>(&xs[(tap * PT + pl) * 32 + part * 8]) = sx[i];
            }
        }
        __syncthreads();
        if (TAPS == 27) {
#pragma unroll
            for (int ks = 0; ks < PT / 16; ks++) {
                const int f0 = ks * 16 + 8 * h;
                const bf16x8 bfrag = tr_frag(ds + f0 * 32 + lane_off);
#pragma unroll
                for (int t = 0; t < NACC; t++) {
                    // tap 27 (wave 3, t = 6) recomputes tap 26 and is dropped at the end: no branches between MFMAs
                    const int tap = wave + 4 * t < 27 ? wave + 4 * t : 26;
                    const bf16x8 afrag = tr_frag(xs + (tap * PT + f0) * 32 + lane_off);
                    acc[t] = RU3D_MFMA_32X32X16(afrag, bfrag, acc[t], 0, 0, 0);
                }
            }
        } else {
#pragma unroll
            for (int kk = 0; kk < PT / 64; kk++) {
                const int f0 = (wave * (PT / 64) + kk) * 16 + 8 * h;
                const bf16x8 bfrag = tr_frag(ds + f0 * 32 + lane_off);
                const bf16x8 afrag = tr_frag(xs + f0 * 32 + lane_off);
                acc[0] = RU3D_MFMA_32X32X16(afrag, bfrag, acc[0], 0, 0, 0);
            }
        }
    }
    // slabs: TAPS == 27: one per workgroup (chunk = blockIdx.x); TAPS == 1: one per wave (chunk = 4 blockIdx.x + wave)
#pragma unroll
    for (int t = 0; t < NACC; t++) {
        const int tap = (TAPS == 27) ? wave + 4 * t : 0;
        if (tap < TAPS) {
            const int64_t chunk = (TAPS == 27) ? blockIdx.x : (int64_t)blockIdx.x * 4 + wave;
            float* pp = a.part + (chunk * TAPS + tap) * a.Cin * a.Cout;
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const int ci = cit * 32 + (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5);
                const int co = cot * 32 + (lane & 31);
                pp[(int64_t)ci * a.Cout + co] = acc[t][i];
            }
        }
    }
}

static int staged_groups(const WgradGeom& g) {
    const int64_t P = (int64_t)g.N * g.Do * g.Ho * g.Wo;
    const int pt = (g.k == 3) ? 32 : 256;
    const int64_t ntiles = (P + pt - 1) / pt;
    const int pairs = (g.Cin / 32) * (g.Cout / 32);
    int64_t G = 1024 / pairs;
    if (G < 1) G = 1;
    if (G > ntiles) G = ntiles;
    return (int)G;
}

bool mfma_wgrad_eligible(const WgradGeom& g, int dtype) {
    const bool form = (g.k == 3 && (g.stride == 1 || g.stride == 2)) || g.k == 1;
    return dtype == RU3D_BF16 && form && (g.Cin % 32) == 0 && (g.Cout % 32) == 0 && (g.ldx % 8) == 0 &&
           (g.lddy % 8) == 0;
}

static int wgrad_tile_groups(const WgradGeom& g, int td, int th, int tw) {
    const int64_t ntiles = (int64_t)g.N * ((g.Do + td - 1) / td) * ((g.Ho + th - 1) / th) * ((g.Wo + tw - 1) / tw);
    const int pairs = (g.Cin / 32) * (g.Cout / 32);
    int64_t G = 512 / pairs;      // 512 workgroups in all: the tuned optimum (256 / 384 / 768 all slower, round 3)
    if (G < 1) G = 1;
    if (G > ntiles) G = ntiles;
    // one workgroup per CU already and few tiles each (512 -> 512 on 8^3: 256 pairs x 4 tiles): a single workgroup per
    // pair writes the gradient itself (RU3D_WGRAD_DIRECT=0: two slabs + the reduce pass)
    static const int direct = ru3d_env_int("RU3D_WGRAD_DIRECT", 1);
    if (direct && pairs >= 224 && ntiles <= 8) G = 1;
    return (int)G;
}

static int wgrad_staged_launch(const void* x, const void* dy, float* dw, void* ws, const WgradGeom& g, const WgradPlan& p,
                               hipStream_t st) {
    StagedWgradArgs a;
    a.x = (const bf16*)x;
    a.dy = (const bf16*)dy;
    a.part = (float*)ws;
    a.N = g.N; a.Di = g.Di; a.Hi = g.Hi; a.Wi = g.Wi; a.Do = g.Do; a.Ho = g.Ho; a.Wo = g.Wo;
    a.Cin = g.Cin; a.Cout = g.Cout; a.ldx = g.ldx; a.lddy = g.lddy;
    a.stride = g.stride; a.pad = g.pad;
    a.x_cseg = g.x_cseg; a.x_segstride = g.x_segstride;
    a.P = (int64_t)g.N * g.Do * g.Ho * g.Wo;
    const int64_t ntiles = (a.P + p.pt - 1) / p.pt;
    if (ntiles > 0x7fffffff) return ru3d_fail(-1, "wgrad_staged: too many tiles");
    a.ntiles = (int)ntiles;
    a.G = g.k == 3 ? p.groups : p.groups / 4;      // 1x1x1: a slab per wave
    dim3 grid(a.G, (g.Cin / 32) * (g.Cout / 32));
    if (g.k == 3) hipLaunchKernelGGL((wgrad_staged_mfma_kernel<27, 32>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((wgrad_staged_mfma_kernel<1, 256>), grid, dim3(256), 0, st, a);
    int rc = ru3d_check_launch(p.name);
    if (rc) return rc;
    return wgrad_reduce_launch((const float*)ws, dw, p.groups, g.taps, g.Cin, g.Cout, g.s_o, g.s_i, st);
}

static int wgrad_tile_launch(const void* x, const void* dy, float* dw, void* ws, const WgradGeom& g, const WgradPlan& p,
                             hipStream_t st) {
    MfmaWgradArgs a;
    a.x = (const bf16*)x;
    a.dy = (const bf16*)dy;
    a.part = (float*)ws;
    a.N = g.N; a.D = g.Do; a.H = g.Ho; a.W = g.Wo;
    a.Cin = g.Cin; a.Cout = g.Cout; a.ldx = g.ldx; a.lddy = g.lddy;
    a.tiles_d = (g.Do + p.td - 1) / p.td;
    a.tiles_h = (g.Ho + p.th - 1) / p.th;
    a.tiles_w = (g.Wo + p.tw - 1) / p.tw;
    a.ntiles = g.N * a.tiles_d * a.tiles_h * a.tiles_w;
    a.G = p.groups;
    // the gradient in the Conv3d layout [co][ci][27], 16-byte aligned: a lone workgroup per pair stores it directly
    a.dw = (p.direct && aligned_to(dw, 16)) ? dw : nullptr;
    dim3 grid(a.G, (g.Cin / 32) * (g.Cout / 32));
    if (p.tw == 32)
        hipLaunchKernelGGL((wgrad3_s1_mfma_kernel<2, 4, 32>), grid, dim3(256), 0, st, a);
    else if (p.tw == 16)
        hipLaunchKernelGGL((wgrad3_s1_mfma_kernel<2, 8, 16>), grid, dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL((wgrad3_s1_mfma_kernel<4, 8, 8>), grid, dim3(256), 0, st, a);
    int rc = ru3d_check_launch(p.name);
    if (rc || a.dw) return rc;
    return wgrad_reduce_launch((const float*)ws, dw, a.G, 27, g.Cin, g.Cout, g.s_o, g.s_i, st);
}

// ---- the plan: which family takes (geometry, dtype), its decomposition, what the queries report
static void wgrad_refuse(WgradPlan& p, const char* why) {
    p.family = 0;
    p.can_pair = false;
    p.refusal = why;
}

WgradPlan wgrad_plan(const WgradGeom& g, int dtype) {
    WgradPlan p;
    // a split (planar concat) x: only the MFMA families, and among them only sliding and staged
    if (!g.x_cseg && (stem_wgrad_plan(g, dtype, &p) || head_wgrad_plan(g, dtype, &p))) return p;
    const size_t slab = (size_t)g.taps * g.Cin * g.Cout * sizeof(float);
    if (!mfma_wgrad_eligible(g, dtype)) {
        if (g.x_cseg) {
            wgrad_refuse(p, "conv3d_wgrad: no kernel takes a split x for this shape / dtype");
            return p;
        }
        p.family = WG_GENERIC;
        p.groups = wgrad_generic_chunks(g);
        p.ws_bytes = p.groups * slab;
        snprintf(p.name, sizeof p.name, "wgrad_generic");
        return p;
    }
    const bool seg_ok = !g.x_cseg || (g.x_cseg % 32) == 0;      // segments of whole 32-channel tiles
    size_t other;                                               // the family that does not run, see ws_bytes
    if (g.k == 3 && g.stride == 1) {                            // the halo forms: sliding, else tiles
        p.tw = s1_width_class(g.Do, g.Ho, g.Wo);
        s1_tile_dims(p.tw, 2, &p.td, &p.th);
        const int tile_groups = wgrad_tile_groups(g, p.td, p.th, p.tw);
        other = tile_groups * slab;
        if (wgrad_slide_plan(g, &p)) {
            p.family = WG_SLIDE;
            p.can_pair = true;
            if (!seg_ok) wgrad_refuse(p, "wgrad_slide: split x needs segments of whole 32-channel tiles");
        } else {
            p.family = WG_S1_TILE;
            p.groups = tile_groups;
            p.direct = p.groups == 1 && g.s_i == 27 && g.s_o == (int64_t)g.Cin * 27;
            snprintf(p.name, sizeof p.name, "wgrad3_s1_mfma<%d,%d,%d>", p.td, p.th, p.tw);
            if (g.x_cseg) wgrad_refuse(p, "wgrad_mfma: only the sliding kernel takes a split x");
        }
    } else {                                                    // stride 2, ConvTranspose, 1x1x1: s2, else staged
        const int staged_slabs = staged_groups(g) * (g.k == 1 ? 4 : 1);
        other = staged_slabs * slab;
        if (wgrad_s2_plan(g, &p)) {
            p.family = WG_S2;
            p.can_pair = p.dma;
            if (g.x_cseg) wgrad_refuse(p, "wgrad_mfma: no stride-2 kernel takes a split x");
        } else {
            p.family = WG_STAGED;
            p.groups = staged_slabs;
            p.pt = g.k == 3 ? 32 : 256;
            snprintf(p.name, sizeof p.name, "wgrad_staged_mfma<%d,%d>", g.taps, p.pt);
            if (!seg_ok) wgrad_refuse(p, "wgrad_staged: split x needs segments of whole 32-channel tiles");
        }
    }
    p.ws_bytes = p.groups * slab > other ? p.groups * slab : other;
    if (p.can_pair) p.pair_ws_bytes = (size_t)p.groups * (g.taps + 1) * g.Cin * g.Cout * sizeof(float);
    return p;
}

// ---- the one consumer: launch-time checks, then the family's launcher
int wgrad_launch(const WgradPlan& p, const void* x, const void* dy, float* dw, void* ws, size_t ws_bytes,
                 const WgradGeom& g, int dtype, hipStream_t st, const void* dy2, int lddy2, float* dw2, float* db) {
    if (!p.family) return ru3d_fail(-1, "%s", p.refusal ? p.refusal : "wgrad: no kernel takes this shape / dtype");
    if (dy2 && !p.can_pair) return ru3d_fail(-1, "wgrad: no pair form for this shape");
    if (db && !p.gives_bias) return ru3d_fail(-1, "stem_wgrad: no bias gradient from this form");
    const size_t need = dy2 ? p.pair_ws_bytes : p.ws_bytes;
    if (!ws || ws_bytes < need) {
        if (dy2) return ru3d_fail(-1, "conv3d_wgrad_pair: workspace too small");
        if (p.family <= WG_HEAD) return ru3d_fail(-1, "%s: workspace too small", p.family == WG_HEAD ? "head_wgrad" : "stem_wgrad");
        return ru3d_fail(-1, "%s: workspace too small (%zu < %zu)", p.family == WG_GENERIC ? "wgrad" : "wgrad_mfma", ws_bytes, need);
    }
    const bool mfma = p.family >= WG_SLIDE && p.family <= WG_STAGED;
    if (mfma && (!aligned_to(x, 16) || !aligned_to(dy, 16) || !aligned_to(dy2, 16)))
        return ru3d_fail(-1, "wgrad_mfma: operands must be 16-byte aligned");
    switch (p.family) {
        case WG_STEM_MFMA:
        case WG_STEM: return stem_wgrad_launch(x, dy, dw, db, ws, g, p, dtype, st);
        case WG_HEAD: return head_wgrad_launch(x, dy, dw, ws, g, p, dtype, st);
        case WG_SLIDE: return wgrad_slide_launch(x, dy, dy2, lddy2, dw, dw2, ws, g, p, st);
        case WG_S1_TILE: return wgrad_tile_launch(x, dy, dw, ws, g, p, st);
        case WG_S2: return wgrad_s2_launch(x, dy, dy2, lddy2, dw, dw2, ws, g, p, st);
        case WG_STAGED: return wgrad_staged_launch(x, dy, dw, ws, g, p, st);
        default: return wgrad_generic_launch(x, dy, dw, ws, p.groups, g, dtype, st);
    }
}

}  // namespace RU3D_NS
