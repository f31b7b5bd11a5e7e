// The "direct" MFMA conv family (v_mfma_f32_32x32x16, fp32 accumulate): every data-movement form with MFMA-friendly channel
// counts that conv3_s1_plan does not take - the 1x1x1 convs, the 3x3x3 stride-2 gather and the transposed form.
// conv_direct_plan decides, conv_direct_launch launches (conv.h: ConvDirectPlan).
#include "common.h"
#include "conv.h"

#include <type_traits>

namespace RU3D_NS {

// "Direct" MFMA conv: the activation fragment of every (tap, k-step) is loaded straight from global memory
// (16 bytes per lane, L1/L2 absorb the tap re-reads), no LDS tile.  Covers every remaining data-movement
// form of the U-Net with MFMA-friendly channel counts: 1x1x1 convs (stride 1/2), 3x3x3 stride-2 gather
// (pooling conv, ConvTranspose dgrad) and the transposed form (ConvTranspose fwd, stride-2 conv dgrad).
// Transposed form: a workgroup owns 32 half-resolution positions x the 8 output parity classes; a wave's
// column tile holds ONE parity class, so only that class' taps (1/2/4/8 of 27) are issued - no masked MFMAs.
struct DirectArgs {
    const bf16* x;
    const bf16x8* w;
    const float* bias;
    const bf16* res;
    bf16* y;
    int N, Di, Hi, Wi, Do, Ho, Wo;
    int Cin, Cout, ldx, ldy, ldr;
    int k, stride, pad, flip, zero_far;
    int hd, hh, hw;          // transposed form: half-resolution extents ceil(Do/2)...
    int64_t total;           // gather: N*Do*Ho*Wo ; transposed: N*hd*hh*hw
    int rows16;              // y (and res) allow 16-byte row pieces: pitch % 8 == 0, base 16-byte aligned
};

// Epilogue of one 32-position column tile held in 32x32x16 accumulators (lane -> position lane & 31, output channels
// 8 q + 4 (lane >> 5) + i of tile t).  Written straight from that layout, a store instruction puts 8 bytes per lane at the
// pitch of a voxel row: a 64- or 128-byte row arrives as 4-8 partial write requests.  Through a wave-private fp32 LDS
// patch the lanes are re-dealt row-major - NT * 4 lanes x 16 bytes cover a position's NT * 32 channels - so every
// request carries a whole row (and consecutive positions, where the form has them, one contiguous run).  Same
// arithmetic as the direct form: (acc + bias) [zeroed on the far planes] + residual, rounded once.
template <int NT>
__device__ __forceinline__ void tile_epilogue_rows(const f32x16 (&acc)[NT], float* patch, int lane, int64_t vox_lane,
                                                   bool far_lane, const float* bias, const bf16* res, int ldr, bf16* y,
                                                   int ldy, int co_blk) {
    constexpr int PP = NT * 32 + 4;          // floats per patch row
    constexpr int PPR = NT * 4;              // 8-channel pieces per row
#pragma unroll
    for (int t = 0; t < NT; t++)
#pragma unroll
        for (int q = 0; q < 4; q++) {
            f32x4 v = {acc[t][q * 4], acc[t][q * 4 + 1], acc[t][q * 4 + 2], acc[t][q * 4 + 3]};
            if (bias) v += *reinterpret_cast<const f32x4*>(bias + co_blk + t * 32 + 8 * q + 4 * (lane >> 5));
            if (far_lane) v = f32x4{0.f, 0.f, 0.f, 0.f};
            *reinterpret_cast<f32x4*>(patch + (lane & 31) * PP + t * 32 + 8 * q + 4 * (lane >> 5)) = v;
        }
    const int vlo = (int)(vox_lane & 0xffffffff), vhi = (int)(vox_lane >> 32);
#pragma unroll
    for (int it = 0; it < 32 * PPR / 64; it++) {
        const int p = lane + 64 * it;
        const int row = p / PPR, chunk = p % PPR;
        const int64_t vox = ((int64_t)__shfl(vhi, row, 64) << 32) | (uint32_t)__shfl(vlo, row, 64);
        const f32x4 lo = *reinterpret_cast<const f32x4*>(patch + row * PP + chunk * 8);
        const f32x4 hi = *reinterpret_cast<const f32x4*>(patch + row * PP + chunk * 8 + 4);
        float v[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        if (vox >= 0) {
            if (res) {
                float r[8];
                load_vec<bf16, 8>(res + vox * ldr + co_blk + chunk * 8, r);
#pragma unroll
                for (int i = 0; i < 8; i++) v[i] += r[i];
            }
            store_vec<bf16, 8>(y + vox * ldy + co_blk + chunk * 8, v);
        }
    }
}

template <int NT, bool TRANSPOSED>
__global__ __launch_bounds__(256) void conv_direct_mfma_kernel(DirectArgs a) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int NTT = a.Cout / 32, KS = a.Cin / 16;
    const int co_blk = blockIdx.y * (NT * 32);
    const int taps = a.k * a.k * a.k;

    f32x16 acc[2][NT];
#pragma unroll
    for (int m = 0; m < 2; m++)
#pragma unroll
        for (int t = 0; t < NT; t++)
#pragma unroll
            for (int i = 0; i < 16; i++) acc[m][t][i] = 0.f;

    int n_[2], od[2], oh[2], ow[2];
    bool valid[2];
    int ba[2], bb[2], bc[2];   // transposed: half-res coordinates
#pragma unroll
    for (int m = 0; m < 2; m++) {
        if (!TRANSPOSED) {
            const int64_t v = (int64_t)blockIdx.x * 256 + (wave * 2 + m) * 32 + (lane & 31);
            valid[m] = v < a.total;
            const int64_t vv = valid[m] ? v : 0;
            ow[m] = (int)(vv % a.Wo);
            int64_t t = vv / a.Wo;
            oh[m] = (int)(t % a.Ho);
            t /= a.Ho;
            od[m] = (int)(t % a.Do);
            n_[m] = (int)(t / a.Do);
            ba[m] = bb[m] = bc[m] = 0;
        } else {
            const int64_t hp = (int64_t)blockIdx.x * 32 + (lane & 31);
            const bool ok = hp < a.total;
            const int64_t vv = ok ? hp : 0;
            bc[m] = (int)(vv % a.hw);
            int64_t t = vv / a.hw;
            bb[m] = (int)(t % a.hh);
            t /= a.hh;
            ba[m] = (int)(t % a.hd);
            n_[m] = (int)(t / a.hd);
            const int cl = wave * 2 + m;
            od[m] = 2 * ba[m] + (cl >> 2);
            oh[m] = 2 * bb[m] + ((cl >> 1) & 1);
            ow[m] = 2 * bc[m] + (cl & 1);
            valid[m] = ok && od[m] < a.Do && oh[m] < a.Ho && ow[m] < a.Wo;
        }
    }

#pragma unroll
    for (int m = 0; m < 2; m++) {
        const int cl = wave * 2 + m;   // parity class of this column tile (transposed form)
        for (int kd = 0; kd < a.k; kd++) {
            int id, qd = 0;
            if (TRANSPOSED) {
                qd = (cl >> 2) + a.pad - kd;
                if (qd & 1) continue;              // wave-uniform: this tap does not feed this parity class
                id = ba[m] + (qd >> 1);
            } else {
                id = od[m] * a.stride + kd - a.pad;
            }
            for (int kh = 0; kh < a.k; kh++) {
                int ih;
                if (TRANSPOSED) {
                    const int qh = ((cl >> 1) & 1) + a.pad - kh;
                    if (qh & 1) continue;
                    ih = bb[m] + (qh >> 1);
                } else {
                    ih = oh[m] * a.stride + kh - a.pad;
                }
                for (int kw = 0; kw < a.k; kw++) {
                    int iw;
                    if (TRANSPOSED) {
                        const int qw = (cl & 1) + a.pad - kw;
                        if (qw & 1) continue;
                        iw = bc[m] + (qw >> 1);
                    } else {
                        iw = ow[m] * a.stride + kw - a.pad;
                    }
                    const int tap = (kd * a.k + kh) * a.k + kw;
                    const int wtap = a.flip ? taps - 1 - tap : tap;
                    const bool inb = valid[m] && id >= 0 && id < a.Di && ih >= 0 && ih < a.Hi && iw >= 0 && iw < a.Wi;
                    const bf16* xp = a.x + ((((int64_t)n_[m] * a.Di + (inb ? id : 0)) * a.Hi + (inb ? ih : 0)) * a.Wi +
                                            (inb ? iw : 0)) * a.ldx + (lane >> 5) * 8;
                    const bf16x8* wrow = a.w + ((int64_t)wtap * KS * NTT + blockIdx.y * NT) * 64 + lane;
#pragma unroll 2
                    for (int ks = 0; ks < KS; ks++) {
                        bf16x8 xb = {0, 0, 0, 0, 0, 0, 0, 0};
                        if (inb) xb = *reinterpret_cast<const bf16x8*>(xp + ks * 16);
#pragma unroll
                        for (int t = 0; t < NT; t++) {
                            const bf16x8 wa = wrow[((int64_t)ks * NTT + t) * 64];
                            acc[m][t] = RU3D_MFMA_32X32X16(wa, xb, acc[m][t], 0, 0, 0);
                        }
                    }
                }
            }
        }
    }

#pragma unroll
    for (int m = 0; m < 2; m++) {
        if (!valid[m]) continue;
        const int64_t vox = (((int64_t)n_[m] * a.Do + od[m]) * a.Ho + oh[m]) * a.Wo + ow[m];
        const bool far = a.zero_far && (od[m] == a.Do - 1 || oh[m] == a.Ho - 1 || ow[m] == a.Wo - 1);
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
                if (far) {
#pragma unroll
                    for (int i = 0; i < 4; i++) v[i] = 0.f;
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

// Gather form on the large levels (3x3x3 stride-2 pooling conv / ConvTranspose input gradient, 1x1x1 convs), second
// take: the kernel above recomputes a lane's input coordinates and bounds for every (tap, k-step) and reloads the
// weight fragment for each of its two column tiles.  Here the per-lane work of an iteration is one bit test and one
// 64-bit add (the lane's base address and its 27-bit mask of in-range taps are computed once; the tap's address delta
// is wave-uniform; out-of-range lanes read a 16-byte zero block), the two column tiles share every weight fragment, and
// the fragments of iteration j + 1 are in flight while iteration j's MFMAs issue.
// 16 zero bytes in the code object's data segment: out-of-range lanes load them instead of branching
__device__ __attribute__((aligned(16))) bf16 g_zero16[8];

template <int NT, int RD>
__global__ __launch_bounds__(256) void conv_gather_mfma_kernel(DirectArgs a) {
    const bf16* const zero16 = g_zero16;
    __shared__ __attribute__((aligned(16))) float patch_s[4][32 * (NT * 32 + 4)];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int NTT = a.Cout / 32, KS = a.Cin / 16;
    const int co_blk = blockIdx.y * (NT * 32);
    const int taps = a.k * a.k * a.k;

    int n_[2], od[2], oh[2], ow[2];
    bool valid[2];
    const bf16* xbase[2];
    uint32_t mask[2];
#pragma unroll
    for (int m = 0; m < 2; m++) {
        const int64_t v = (int64_t)blockIdx.x * 256 + (wave * 2 + m) * 32 + (lane & 31);
        valid[m] = v < a.total;
        const int64_t vv = valid[m] ? v : 0;
        ow[m] = (int)(vv % a.Wo);
        int64_t t = vv / a.Wo;
        oh[m] = (int)(t % a.Ho);
        t /= a.Ho;
        od[m] = (int)(t % a.Do);
        n_[m] = (int)(t / a.Do);
        const int id0 = od[m] * a.stride - a.pad, ih0 = oh[m] * a.stride - a.pad, iw0 = ow[m] * a.stride - a.pad;
        // address of tap (0,0,0) - may lie outside the tensor, only dereferenced for taps whose mask bit is set
        xbase[m] = a.x + ((((int64_t)n_[m] * a.Di + id0) * a.Hi + ih0) * a.Wi + iw0) * (int64_t)a.ldx + (lane >> 5) * 8;
        uint32_t mk = 0;
        for (int kd = 0; kd < a.k; kd++)
            for (int kh = 0; kh < a.k; kh++)
                for (int kw = 0; kw < a.k; kw++) {
                    const int id = id0 + kd, ih = ih0 + kh, iw = iw0 + kw;
                    const bool inb = valid[m] && id >= 0 && id < a.Di && ih >= 0 && ih < a.Hi && iw >= 0 && iw < a.Wi;
                    mk |= (inb ? 1u : 0u) << ((kd * a.k + kh) * a.k + kw);
                }
        mask[m] = mk;
    }

    f32x16 acc[2][NT];
#pragma unroll
    for (int m = 0; m < 2; m++)
#pragma unroll
        for (int t = 0; t < NT; t++)
#pragma unroll
            for (int i = 0; i < 16; i++) acc[m][t][i] = 0.f;

    const int T = taps * KS;
    // RD iterations of fragments in flight (one iteration of prefetch until round 4: every iteration then waited ~500
    // cycles for its L2 hits behind 128 cycles of MFMA - 216 iterations x 0.25 us were the 54 us of the 128 -> 256 conv at
    // 32^3).  The (tap, k-step) counters advance with the fetches (wave-uniform, no division in the loop); iterations past
    // T load the zero block and the last weight fragment again, so the ring body has no branch and the waits stay counted.
    // RD = 6 for the 3x3x3 forms; the 1x1x1 forms (4-32 iterations, HBM-bound on the large levels) keep RD = 2.
    int f_j = 0, f_tap = 0, f_ks = 0, f_kw = 0, f_kh = 0, f_kd = 0;
    auto fetch = [&](bf16x8 (&xb)[2], bf16x8 (&wa)[NT]) {
        const bool live = f_j < T;
        const int64_t delta = (((int64_t)f_kd * a.Hi + f_kh) * a.Wi + f_kw) * a.ldx + f_ks * 16;
        const int wtap = a.flip ? taps - 1 - f_tap : f_tap;
#pragma unroll
        for (int m = 0; m < 2; m++) {
            const bf16* p = (live && ((mask[m] >> f_tap) & 1u)) ? xbase[m] + delta : zero16;
            xb[m] = *reinterpret_cast<const bf16x8*>(p);
        }
        const bf16x8* wrow = a.w + (((int64_t)wtap * KS + f_ks) * NTT + blockIdx.y * NT) * 64 + lane;
#pragma unroll
        for (int t = 0; t < NT; t++) wa[t] = wrow[t * 64];
        if (f_j + 1 < T) {
            f_ks++;
            if (f_ks == KS) {
                f_ks = 0;
                f_tap++;
                f_kw++;
                if (f_kw == a.k) {
                    f_kw = 0;
                    f_kh++;
                    if (f_kh == a.k) {
                        f_kh = 0;
                        f_kd++;
                    }
                }
            }
        }
        f_j++;
    };
    {
        bf16x8 xr[RD][2], wr[RD][NT];
#pragma unroll
        for (int r = 0; r < RD; r++) fetch(xr[r], wr[r]);
        for (int j = 0; j < T; j += RD) {
#pragma unroll
            for (int r = 0; r < RD; r++) {
#pragma unroll
                for (int t = 0; t < NT; t++)
#pragma unroll
                    for (int m = 0; m < 2; m++)
                        acc[m][t] = RU3D_MFMA_32X32X16(wr[r][t], xr[r][m], acc[m][t], 0, 0, 0);
                fetch(xr[r], wr[r]);
            }
        }
    }

    if (a.rows16) {
#pragma unroll
        for (int m = 0; m < 2; m++) {
            const int64_t vox = (((int64_t)n_[m] * a.Do + od[m]) * a.Ho + oh[m]) * a.Wo + ow[m];
            const bool far = a.zero_far && (od[m] == a.Do - 1 || oh[m] == a.Ho - 1 || ow[m] == a.Wo - 1);
            tile_epilogue_rows<NT>(acc[m], patch_s[wave], lane, valid[m] ? vox : -1, far, a.bias, a.res, a.ldr, a.y, a.ldy,
                                   co_blk);
        }
        return;
    }
#pragma unroll
    for (int m = 0; m < 2; m++) {
        if (!valid[m]) continue;
        const int64_t vox = (((int64_t)n_[m] * a.Do + od[m]) * a.Ho + oh[m]) * a.Wo + ow[m];
        const bool far = a.zero_far && (od[m] == a.Do - 1 || oh[m] == a.Ho - 1 || ow[m] == a.Wo - 1);
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
                if (far) {
#pragma unroll
                    for (int i = 0; i < 4; i++) v[i] = 0.f;
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

// The same forms on the deep levels (8^3 .. 16^3 voxels, hundreds of channels): one 256-voxel workgroup per 64 couts
// leaves tens of workgroups, each walking thousands of dependent (load, MFMA) pairs.  Here a workgroup owns ONE
// 32-voxel column tile (transposed form: 32 half-resolution positions of one parity class, blockIdx.z) x NT cout
// tiles, its 4 waves split the (tap, k-step) iterations, every wave keeps the next iteration's fragments in flight,
// and the four partial tiles are summed through LDS in a fixed order before the fused bias / residual / store.
template <int NT, bool TRANSPOSED, int RD>
__global__ __launch_bounds__(256) void conv_direct_ksplit_kernel(DirectArgs a) {
    __shared__ float red[4][NT][64][17];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int NTT = a.Cout / 32, KS = a.Cin / 16;
    const int co_blk = blockIdx.y * (NT * 32);
    const int taps = a.k * a.k * a.k;
    const int cl = TRANSPOSED ? (int)blockIdx.z : 0;

    // this lane's output voxel (column of the MFMA tile)
    int n_, od, oh, ow, ba = 0, bb = 0, bc = 0;
    bool valid;
    {
        const int64_t v = (int64_t)blockIdx.x * 32 + (lane & 31);
        const bool ok = v < a.total;
        const int64_t vv = ok ? v : 0;
        if (!TRANSPOSED) {
            ow = (int)(vv % a.Wo);
            int64_t t = vv / a.Wo;
            oh = (int)(t % a.Ho);
            t /= a.Ho;
            od = (int)(t % a.Do);
            n_ = (int)(t / a.Do);
            valid = ok;
        } else {
            bc = (int)(vv % a.hw);
            int64_t t = vv / a.hw;
            bb = (int)(t % a.hh);
            t /= a.hh;
            ba = (int)(t % a.hd);
            n_ = (int)(t / a.hd);
            od = 2 * ba + (cl >> 2);
            oh = 2 * bb + ((cl >> 1) & 1);
            ow = 2 * bc + (cl & 1);
            valid = ok && od < a.Do && oh < a.Ho && ow < a.Wo;
        }
    }
    // taps that feed this tile, per axis: gather form all k; transposed form those with (class bit + pad - k) even
    int nkd, nkh, nkw, k0d, k0h, k0w, kstep;
    if (!TRANSPOSED) {
        nkd = nkh = nkw = a.k;
        k0d = k0h = k0w = 0;
        kstep = 1;
    } else {
        auto axis = [&](int bit, int& nk, int& k0) {
            k0 = (bit + a.pad) & 1;                 // first k with the right parity
            nk = k0 < a.k ? (a.k - k0 + 1) / 2 : 0;
        };
        axis(cl >> 2, nkd, k0d);
        axis((cl >> 1) & 1, nkh, k0h);
        axis(cl & 1, nkw, k0w);
        kstep = 2;
    }
    const int T = nkd * nkh * nkw * KS;                       // iterations of this tile
    const int j_lo = (T * wave) / 4, j_hi = (T * (wave + 1)) / 4;

    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; t++)
#pragma unroll
        for (int i = 0; i < 16; i++) acc[t][i] = 0.f;

    // Fragments of iteration j: the (tap, k-step) counters advance with j (wave-uniform: scalar unit), no divisions in the
    // loop.  An iteration past the end re-reads the last valid one with a zero activation fragment (its MFMAs add zero): the
    // ring below then has no branch in its body and the compiler's vmcnt waits stay counted.
    // The ring is RD iterations deep: with one iteration of prefetch (rounds 1-3) every step waited ~500 cycles for an L2
    // hit behind 64 cycles of MFMA - 108 steps x 0.4 us were the whole 45-58 us of these launches.  RD = 8 for the 3x3x3
    // forms, 2 for the 1x1x1 forms (4-8 iterations per wave: a deeper ring would be mostly padding).
    int f_ks, f_kw, f_kh, f_kd, f_j;         // state of the NEXT fetch
    {
        f_j = j_lo;
        f_ks = j_lo % KS;
        int tq = j_lo / KS;
        f_kw = tq % nkw;
        tq /= nkw;
        f_kh = tq % nkh;
        f_kd = tq / nkh;
    }
    auto fetch = [&](bf16x8& xb, bf16x8 (&wa)[NT]) {
        const bool live = f_j < j_hi;
        const int ks = f_ks;
        const int kw = k0w + kstep * f_kw, kh = k0h + kstep * f_kh, kd = k0d + kstep * f_kd;
        int id, ih, iw;
        if (TRANSPOSED) {
            id = ba + (((cl >> 2) + a.pad - kd) >> 1);
            ih = bb + ((((cl >> 1) & 1) + a.pad - kh) >> 1);
            iw = bc + (((cl & 1) + a.pad - kw) >> 1);
        } else {
            id = od * a.stride + kd - a.pad;
            ih = oh * a.stride + kh - a.pad;
            iw = ow * a.stride + kw - a.pad;
        }
        const int tap = (kd * a.k + kh) * a.k + kw;
        const int wtap = a.flip ? taps - 1 - tap : tap;
        const bool inb = live && valid && id >= 0 && id < a.Di && ih >= 0 && ih < a.Hi && iw >= 0 && iw < a.Wi;
        // out-of-range lanes load a 16-byte zero block: no select behind the load (the compiler gathered such selects at
        // the top of the unrolled ring body, i.e. waited for the youngest load there)
        const bf16* xp = inb ? a.x + ((((int64_t)n_ * a.Di + id) * a.Hi + ih) * a.Wi + iw) * a.ldx + (lane >> 5) * 8 + ks * 16
                             : (const bf16*)g_zero16;
        xb = *reinterpret_cast<const bf16x8*>(xp);
        const bf16x8* wrow = a.w + (((int64_t)wtap * KS + ks) * NTT + blockIdx.y * NT) * 64 + lane;
#pragma unroll
        for (int t = 0; t < NT; t++) wa[t] = wrow[t * 64];
        if (live && f_j + 1 < j_hi) {         // advance (the last valid iteration is kept for the padding fetches)
            f_ks++;
            if (f_ks == KS) {
                f_ks = 0;
                f_kw++;
                if (f_kw == nkw) {
                    f_kw = 0;
                    f_kh++;
                    if (f_kh == nkh) {
                        f_kh = 0;
                        f_kd++;
                    }
                }
            }
        }
        f_j++;
    };

    if (j_lo < j_hi) {
        bf16x8 xb[RD], wa[RD][NT];
#pragma unroll
        for (int r = 0; r < RD; r++) fetch(xb[r], wa[r]);
        for (int j = j_lo; j < j_hi; j += RD) {
#pragma unroll
            for (int r = 0; r < RD; r++) {
#pragma unroll
                for (int t = 0; t < NT; t++) acc[t] = RU3D_MFMA_32X32X16(wa[r][t], xb[r], acc[t], 0, 0, 0);
                fetch(xb[r], wa[r]);
            }
        }
    }
#pragma unroll
    for (int t = 0; t < NT; t++)
#pragma unroll
        for (int i = 0; i < 16; i++) red[wave][t][lane][i] = acc[t][i];
    __syncthreads();

    // thread -> (voxel, 8 consecutive couts); D layout: col = lane & 31 (voxel), row = (i & 3) + 8 (i >> 2) + 4 (lane >> 5)
    const int vox_l = tid >> 3, cg = tid & 7;
    if (cg * 8 >= NT * 32) return;
    // re-derive the voxel of column vox_l (it is lane vox_l's voxel)
    const int64_t v2 = (int64_t)blockIdx.x * 32 + vox_l;
    if (v2 >= a.total) return;
    int n2, d2, h2, w2;
    if (!TRANSPOSED) {
        w2 = (int)(v2 % a.Wo);
        int64_t t = v2 / a.Wo;
        h2 = (int)(t % a.Ho);
        t /= a.Ho;
        d2 = (int)(t % a.Do);
        n2 = (int)(t / a.Do);
    } else {
        const int c2 = (int)(v2 % a.hw);
        int64_t t = v2 / a.hw;
        const int b2 = (int)(t % a.hh);
        t /= a.hh;
        const int a2 = (int)(t % a.hd);
        n2 = (int)(t / a.hd);
        d2 = 2 * a2 + (cl >> 2);
        h2 = 2 * b2 + ((cl >> 1) & 1);
        w2 = 2 * c2 + (cl & 1);
        if (d2 >= a.Do || h2 >= a.Ho || w2 >= a.Wo) return;
    }
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; e++) {
        const int co = cg * 8 + e;
        const int t = co >> 5, r = co & 31;
        const int h = (r >> 2) & 1, i = (r & 3) + 4 * (r >> 3);
        const int ln = vox_l + 32 * h;
        v[e] = (red[0][t][ln][i] + red[1][t][ln][i]) + (red[2][t][ln][i] + red[3][t][ln][i]);
    }
    const int c0 = co_blk + cg * 8;
    if (a.bias) {
#pragma unroll
        for (int e = 0; e < 8; e++) v[e] += a.bias[c0 + e];
    }
    if (a.zero_far && (d2 == a.Do - 1 || h2 == a.Ho - 1 || w2 == a.Wo - 1)) {
#pragma unroll
        for (int e = 0; e < 8; e++) v[e] = 0.f;
    }
    const int64_t vox = (((int64_t)n2 * a.Do + d2) * a.Ho + h2) * a.Wo + w2;
    if (a.res) {
#pragma unroll
        for (int e = 0; e < 8; e++) v[e] += (float)a.res[vox * a.ldr + c0 + e];
    }
    // y pitch and base are 8-byte aligned (checked by the launcher); two 4-element stores
    float lo[4] = {v[0], v[1], v[2], v[3]}, hi[4] = {v[4], v[5], v[6], v[7]};
    store_vec<bf16, 4>(a.y + vox * a.ldy + c0, lo);
    store_vec<bf16, 4>(a.y + vox * a.ldy + c0 + 4, hi);
}

// Transposed form (ConvTranspose3d k3 s2 p1 forward, stride-2 conv input gradient) on the large levels through an
// LDS tile: a workgroup owns 128 half-resolution positions (TD x TH x TW) and stages their (TD+1)(TH+1)(TW+1) input
// rows ONCE - all 8 output parity classes read the same 2x2x2 neighbourhoods, so the 27 taps cost one global read
// of the input instead of 27 L1/L2 gathers.  Waves take whole parity classes (8 | 4+2+1 | 4+2 | 4+2 taps); per class
// a wave holds the 4 column tiles of the workgroup, so every weight fragment (global, prefetched one iteration
// ahead) feeds 4 MFMAs per cout tile.  Row pitch Cin*2 + 16 bytes: conflict-free ds_read_b128 over a W-run.
template <int NT, int TD, int TH, int TW>
__global__ __launch_bounds__(256, 2) void convt_tile_mfma_kernel(DirectArgs a) {
    extern __shared__ __attribute__((aligned(16))) bf16 tile_lds[];
    static_assert((TD * TH * TW) % 32 == 0, "whole column tiles");
    constexpr int HD = TD + 1, HH = TH + 1, HW = TW + 1, ROWS = HD * HH * HW;
    constexpr int MT = TD * TH * TW / 32;       // column tiles of 32 positions: every weight fragment feeds MT MFMAs
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int NTT = a.Cout / 32, KS = a.Cin / 16;
    const int pitch = a.Cin + 8;                 // bf16 elements
    const int co_blk = blockIdx.y * (NT * 32);

    // tile origin in half-resolution coordinates
    const int tw_n = (a.hw + TW - 1) / TW, th_n = (a.hh + TH - 1) / TH, td_n = (a.hd + TD - 1) / TD;
    int t = blockIdx.x;
    const int c0 = (t % tw_n) * TW;
    t /= tw_n;
    const int b0 = (t % th_n) * TH;
    t /= th_n;
    const int a0 = (t % td_n) * TD;
    const int n = t / td_n;

    // ---- stage the input rows (zero outside the tensor)
    // eight pieces per thread in flight: written as load -> store per piece the loop ran at one memory round trip per
    // iteration (the store waits for its load), 16-31 of them per tile
    const int ppr = a.Cin / 8;                   // 16-byte pieces per row
    constexpr int SB = 8;
    for (int p0 = tid; p0 < ROWS * ppr; p0 += 256 * SB) {
        bf16x8 v[SB];
        int dst[SB];
#pragma unroll
        for (int u = 0; u < SB; u++) {
            const int p = p0 + 256 * u;
            const bf16x8 z8 = {0, 0, 0, 0, 0, 0, 0, 0};
            v[u] = z8;
            dst[u] = -1;
            if (p < ROWS * ppr) {
                const int r = p / ppr, piece = p - r * ppr;
                const int zc = r % HW, zb = (r / HW) % HH, za = r / (HW * HH);
                const int ia = a0 + za, ib = b0 + zb, ic = c0 + zc;
                dst[u] = r * pitch + piece * 8;
                if (ia < a.Di && ib < a.Hi && ic < a.Wi)
                    v[u] = *reinterpret_cast<const bf16x8*>(a.x + ((((int64_t)n * a.Di + ia) * a.Hi + ib) * a.Wi + ic) * a.ldx + piece * 8);
            }
        }
#pragma unroll
        for (int u = 0; u < SB; u++)
            if (dst[u] >= 0) *reinterpret_cast<bf16x8*>(tile_lds + dst[u]) = v[u];
    }
    __syncthreads();

    // column tile m of the workgroup: positions f = m*32 + (lane & 31)
    int rowm[MT], pa[MT], pb[MT], pc[MT];
#pragma unroll
    for (int m = 0; m < MT; m++) {
        const int f = m * 32 + (lane & 31);
        pc[m] = f % TW;
        pb[m] = (f / TW) % TH;
        pa[m] = f / (TW * TH);
        rowm[m] = ((pa[m] * HH + pb[m]) * HW + pc[m]) * pitch + (lane >> 5) * 8;
    }

    // classes of this wave, heaviest first: {7} | {3, 1, 0} | {5, 2} | {6, 4}   (taps 8 | 4+2+1 | 4+2 | 4+2)
    const int ncls = wave == 0 ? 1 : (wave == 1 ? 3 : 2);
    for (int ci = 0; ci < ncls; ci++) {
        const int cl = wave == 0 ? 7 : wave == 1 ? (ci == 0 ? 3 : (ci == 1 ? 1 : 0)) : wave == 2 ? (ci == 0 ? 5 : 2) : (ci == 0 ? 6 : 4);
        const int bd = cl >> 2, bh = (cl >> 1) & 1, bw = cl & 1;
        // taps of the class per axis: bit 0 -> k = 1 (input offset 0); bit 1 -> k = 0 (offset 1), k = 2 (offset 0)
        const int nkd = 1 + bd, nkh = 1 + bh, nkw = 1 + bw;
        const int T = nkd * nkh * nkw * KS;

        f32x16 acc[MT][NT];
#pragma unroll
        for (int m = 0; m < MT; m++)
#pragma unroll
            for (int tt = 0; tt < NT; tt++)
#pragma unroll
                for (int i = 0; i < 16; i++) acc[m][tt][i] = 0.f;

        auto wfetch = [&](int j, bf16x8 (&wa)[NT], int& roff) {
            const int ks = j % KS;
            int tq = j / KS;
            const int iw = tq % nkw;
            tq /= nkw;
            const int ih = tq % nkh;
            const int idd = tq / nkh;
            // axis with class bit 1: index 0 -> k = 0 (offset 1), index 1 -> k = 2 (offset 0); bit 0: k = 1 (offset 0)
            const int kd = bd ? 2 * idd : 1, kh = bh ? 2 * ih : 1, kw = bw ? 2 * iw : 1;
            const int dd = bd ? 1 - idd : 0, dh = bh ? 1 - ih : 0, dw = bw ? 1 - iw : 0;
            const int tap = (kd * 3 + kh) * 3 + kw;
            const int wtap = a.flip ? 26 - tap : tap;
            const bf16x8* wrow = a.w + (((int64_t)wtap * KS + ks) * NTT + blockIdx.y * NT) * 64 + lane;
#pragma unroll
            for (int tt = 0; tt < NT; tt++) wa[tt] = wrow[tt * 64];
            roff = ((dd * HH + dh) * HW + dw) * pitch + ks * 16;
        };
        auto compute = [&](const bf16x8 (&wa)[NT], int roff) {
            bf16x8 xb[MT];
#pragma unroll
            for (int m = 0; m < MT; m++) xb[m] = *reinterpret_cast<const bf16x8*>(tile_lds + rowm[m] + roff);
#pragma unroll
            for (int m = 0; m < MT; m++)
#pragma unroll
                for (int tt = 0; tt < NT; tt++)
                    acc[m][tt] = RU3D_MFMA_32X32X16(wa[tt], xb[m], acc[m][tt], 0, 0, 0);
        };
        // weight fragments RD iterations ahead (one until round 4: an L2 hit takes longer than the 4-8 MFMAs of an
        // iteration), activation fragments of the next iteration read from LDS in front of this iteration's MFMAs;
        // the fetches past the end repeat the last iteration's (branch-free body, counted waits)
        auto ring = [&](auto rd_tag) {
            constexpr int RD = decltype(rd_tag)::value;
            bf16x8 wq[RD][NT], xq[2][MT];
            int ro[RD];
            int fj = 0;
            auto wnext = [&](bf16x8 (&wa)[NT], int& roff) {
                wfetch(fj < T ? fj : T - 1, wa, roff);
                fj++;
            };
#pragma unroll
            for (int r = 0; r < RD; r++) wnext(wq[r], ro[r]);
#pragma unroll
            for (int m = 0; m < MT; m++) xq[0][m] = *reinterpret_cast<const bf16x8*>(tile_lds + rowm[m] + ro[0]);
            for (int j = 0; j < T; j += RD) {
#pragma unroll
                for (int r = 0; r < RD; r++) {
#pragma unroll
                    for (int m = 0; m < MT; m++)
                        xq[(r + 1) & 1][m] = *reinterpret_cast<const bf16x8*>(tile_lds + rowm[m] + ro[(r + 1) % RD]);
#pragma unroll
                    for (int m = 0; m < MT; m++)
#pragma unroll
                        for (int tt = 0; tt < NT; tt++)
                            acc[m][tt] = RU3D_MFMA_32X32X16(wq[r][tt], xq[r & 1][m], acc[m][tt], 0, 0, 0);
                    wnext(wq[r], ro[r]);
                }
            }
        };
        // (8 deep for the 4-MFMA iterations of the NT = 1 forms: 56 vs 54-55 us - no better)
        if ((T % 4) == 0) {
            ring(std::integral_constant<int, 4>{});
        } else {
            bf16x8 w0[NT], w1[NT];
            int r0, r1;
            wfetch(0, w0, r0);
            int j = 0;
            for (; j + 1 < T; j += 2) {
                wfetch(j + 1, w1, r1);
                compute(w0, r0);
                if (j + 2 < T) wfetch(j + 2, w0, r0);
                compute(w1, r1);
            }
            if (j < T) compute(w0, r0);
        }

        // ---- epilogue of the class: output voxel (2a + bd, 2b + bh, 2c + bw)
#pragma unroll
        for (int m = 0; m < MT; m++) {
            const int od = 2 * (a0 + pa[m]) + bd, oh = 2 * (b0 + pb[m]) + bh, ow = 2 * (c0 + pc[m]) + bw;
            if (od >= a.Do || oh >= a.Ho || ow >= a.Wo) continue;
            const int64_t vox = (((int64_t)n * a.Do + od) * a.Ho + oh) * a.Wo + ow;
            const bool far = a.zero_far && (od == a.Do - 1 || oh == a.Ho - 1 || ow == a.Wo - 1);
#pragma unroll
            for (int tt = 0; tt < NT; tt++) {
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int cc = co_blk + tt * 32 + 8 * q + 4 * (lane >> 5);
                    float v[4];
#pragma unroll
                    for (int i = 0; i < 4; i++) v[i] = acc[m][tt][q * 4 + i];
                    if (a.bias) {
                        const f32x4 b = *reinterpret_cast<const f32x4*>(a.bias + cc);
#pragma unroll
                        for (int i = 0; i < 4; i++) v[i] += b[i];
                    }
                    if (far) {
#pragma unroll
                        for (int i = 0; i < 4; i++) v[i] = 0.f;
                    }
                    if (a.res) {
                        float r[4];
                        load_vec<bf16, 4>(a.res + vox * a.ldr + cc, r);
#pragma unroll
                        for (int i = 0; i < 4; i++) v[i] += r[i];
                    }
                    store_vec<bf16, 4>(a.y + vox * a.ldy + cc, v);
                }
            }
        }
    }
}

template <int NT, int TD, int TH, int TW>
static int launch_convt_tile(const DirectArgs& a, int N, hipStream_t st, const char* name) {
    const int tw_n = (a.hw + TW - 1) / TW, th_n = (a.hh + TH - 1) / TH, td_n = (a.hd + TD - 1) / TD;
    const int64_t nblk = (int64_t)N * td_n * th_n * tw_n;
    if (nblk > 0x7fffffff) return ru3d_fail(-1, "convt_tile: grid too large");
    const size_t lds = (size_t)(TD + 1) * (TH + 1) * (TW + 1) * (a.Cin + 8) * sizeof(bf16);
    auto kern = convt_tile_mfma_kernel<NT, TD, TH, TW>;
    static bool attr_set = false;
    if (!attr_set) {
        if (hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess)
            return ru3d_fail(-1, "convt_tile: cannot raise the dynamic LDS limit");
        attr_set = true;
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)nblk, a.Cout / (NT * 32)), dim3(256), lds, st, a);
    return ru3d_check_launch(name);
}

// ---------------------------------------------------------------------------------------------------------
// Host side of the family: conv_direct_plan decides, conv_direct_launch runs the first choice whose launch-time
// conditions hold (conv.h: ConvDirectPlan).
typedef void (*DirectKernel)(DirectArgs);

// positions the grid is made of (gather: output voxels; transposed: half-resolution positions of 8 parity classes)
static int64_t direct_total(const ConvGeom& g) {
    if (!g.transposed) return (int64_t)g.N * g.Do * g.Ho * g.Wo;
    return (int64_t)g.N * ((g.Do + 1) / 2) * ((g.Ho + 1) / 2) * ((g.Wo + 1) / 2);
}

static void direct_push(ConvDirectPlan& p, int family, bool transposed, int nt, int rd, int td = 0, int th = 0, int tw = 0) {
    p.family = family; p.nt = nt; p.rd = rd; p.td = td; p.th = th; p.tw = tw;
    switch (family) {
        case DIRECT_KSPLIT: snprintf(p.name, sizeof(p.name), "conv_direct_ksplit<%d,%c,%d>", nt, transposed ? 'T' : 'F', rd); break;
        case DIRECT_CONVT_TILE: snprintf(p.name, sizeof(p.name), "convt_tile_mfma<%d,%d,%d,%d>", nt, td, th, tw); break;
        case DIRECT_GATHER: snprintf(p.name, sizeof(p.name), "conv_gather_mfma<%d,%d>", nt, rd); break;
        default: snprintf(p.name, sizeof(p.name), "conv_direct_mfma<%d,T>", nt);
    }
}

ConvDirectPlan conv_direct_plan(const ConvGeom& g) {
    // the family's switches, each read once per process; 0 = that kernel off
    static const int s2_mode = ru3d_env_int("RU3D_CONV_S2", 1), tile_mode = ru3d_env_int("RU3D_CONVT_TILE", 1);
    static const int nt_mode = ru3d_env_int("RU3D_CONVT_NT", 1);      // 0: 64-cout workgroups whatever they leave idle
    ConvDirectPlan p;
    // 1. the large levels' stride-2 forms: LDS-DMA plane ring + producer wave + weights in registers (conv_s2.hip)
    if (s2_mode) g.transposed ? convt_s2_tile_plan(g, &p) : conv_s2_tile_plan(g, &p);
    // 2. the one kernel that takes whatever the launch brings
    const int hh = (g.Ho + 1) / 2, hw = (g.Wo + 1) / 2;
    const int64_t total = direct_total(g), nblk = g.transposed ? (total + 31) / 32 : (total + 255) / 256;
    const int nt = (g.Cout % 64) == 0 ? 2 : 1;
    const bool convt3 = tile_mode && g.transposed && g.k == 3 && g.pad == 1;
    if (nblk > 0x7fffffff) {
        p.refusal = "conv_direct_mfma: grid too large";
    } else if (nblk * (g.Cout / (nt * 32)) < 384) {
        // few, long workgroups: split the reduction over the waves of 32-voxel workgroups instead
        direct_push(p, DIRECT_KSPLIT, g.transposed, nt, g.k >= 3 ? 8 : 2);
    } else if (convt3 && hw >= 24 && g.Cin <= 128) {
        // (TD+1)(TH+1)(TW+1) rows of Cin*2+16 bytes must fit in LDS: Cin <= 256 with the 16-wide tile, 128 with the 32-wide.
        // one cout tile: 256 positions per workgroup (8 column tiles per weight fragment) - the 110 KB of weights a
        // workgroup pulls through its CU's ~10 B/clk are the larger part of what enters it
        if (nt == 1 && g.Cin <= 64 && hh >= 4) direct_push(p, DIRECT_CONVT_TILE, true, 1, 0, 2, 4, 32);
        else direct_push(p, DIRECT_CONVT_TILE, true, nt, 0, 2, 2, 32);
    } else if (convt3 && hw >= 12 && g.Cin <= 256) {
        // 64-cout workgroups only when they still fill the chip (16^3 -> 32^3 at N = 2: 64 tiles)
        const int64_t t16 = (int64_t)g.N * (((g.Do + 1) / 2 + 1) / 2) * ((hh + 3) / 4) * ((hw + 15) / 16);
        const bool wide = nt == 2 && (nt_mode == 0 || t16 * (g.Cout / 64) >= 200);
        direct_push(p, DIRECT_CONVT_TILE, true, wide ? 2 : 1, 0, 2, 4, 16);
    } else if (g.transposed) {
        direct_push(p, DIRECT_T, true, nt, 0);
    } else {
        direct_push(p, DIRECT_GATHER, false, nt, g.k >= 3 ? 6 : 2);
    }
    return p;
}

bool conv_direct_tile_ok(const ConvDirectPlan& p, const ConvGeom& g, const void* x, const void* res, const void* y,
                         const void* partner, int ld_partner) {
    const uintptr_t ux = (uintptr_t)x, ur = (uintptr_t)res, uy = (uintptr_t)y, up = (uintptr_t)partner;
    if (p.tile == S2_TILE_T)      // partner: a second gradient operand on the input grid
        return ((ux | uy | ur | up) % 16) == 0 &&
               (!partner || ((ld_partner % 8) == 0 && (int64_t)g.Di * g.Hi * g.Wi * ld_partner < (1ll << 30)));
    if (p.tile == S2_TILE_G)      // partner: a second output on the output grid; the kernel has no residual form
        return !res && (ux % 16) == 0 && ((uy | up) % 8) == 0 &&
               (!partner || ((ld_partner % 4) == 0 && (int64_t)g.Do * g.Ho * g.Wo * ld_partner < (1ll << 30)));
    return false;
}

template <bool TR> static DirectKernel ksplit_kernel(int nt, int rd) {
    if (rd == 8) return nt == 2 ? conv_direct_ksplit_kernel<2, TR, 8> : conv_direct_ksplit_kernel<1, TR, 8>;
    return nt == 2 ? conv_direct_ksplit_kernel<2, TR, 2> : conv_direct_ksplit_kernel<1, TR, 2>;
}
static DirectKernel gather_kernel(int nt, int rd) {
    if (rd == 6) return nt == 2 ? conv_gather_mfma_kernel<2, 6> : conv_gather_mfma_kernel<1, 6>;
    return nt == 2 ? conv_gather_mfma_kernel<2, 2> : conv_gather_mfma_kernel<1, 2>;
}

int conv_direct_launch(const ConvDirectPlan& p, const void* x, const void* w, const float* bias, const void* res, void* y,
                       const ConvGeom& g, hipStream_t st) {
    if (!p.family) return ru3d_fail(-1, "%s", p.refusal);
    // The fused entry points run the tile kernels under the same plan and the same conv_direct_tile_ok: a block recomputed
    // under activation checkpointing gets the same bits from the plain entry points
    if (conv_direct_tile_ok(p, g, x, res, y))
        return p.tile == S2_TILE_T ? convt_s2_tile_launch(p, x, w, bias, res, y, g, nullptr, nullptr, 0, nullptr, st)
                                   : conv_s2_tile_launch(p, x, w, bias, y, g, nullptr, nullptr, nullptr, nullptr, 0, st);
    DirectArgs a;
    a.x = (const bf16*)x;
    a.w = (const bf16x8*)w;
    a.bias = bias;
    a.res = (const bf16*)res;
    a.y = (bf16*)y;
    a.N = g.N; a.Di = g.Di; a.Hi = g.Hi; a.Wi = g.Wi; a.Do = g.Do; a.Ho = g.Ho; a.Wo = g.Wo;
    a.Cin = g.Cin; a.Cout = g.Cout; a.ldx = g.ldx; a.ldy = g.ldy; a.ldr = g.ldr;
    a.k = g.k; a.stride = g.stride; a.pad = g.pad; a.flip = g.flip; a.zero_far = g.zero_far;
    a.hd = (g.Do + 1) / 2; a.hh = (g.Ho + 1) / 2; a.hw = (g.Wo + 1) / 2;
    a.rows16 = (g.ldy % 8) == 0 && (((uintptr_t)y) % 16) == 0 && (!res || ((g.ldr % 8) == 0 && (((uintptr_t)res) % 16) == 0));
    a.total = direct_total(g);
    if (p.family == DIRECT_CONVT_TILE) {
        if (p.tw == 32 && p.th == 4) return launch_convt_tile<1, 2, 4, 32>(a, g.N, st, p.name);
        if (p.tw == 32) return p.nt == 2 ? launch_convt_tile<2, 2, 2, 32>(a, g.N, st, p.name)
                                         : launch_convt_tile<1, 2, 2, 32>(a, g.N, st, p.name);
        return p.nt == 2 ? launch_convt_tile<2, 2, 4, 16>(a, g.N, st, p.name)
                         : launch_convt_tile<1, 2, 4, 16>(a, g.N, st, p.name);
    }
    DirectKernel kern;
    dim3 grid((unsigned)((a.total + 31) / 32), g.Cout / (p.nt * 32));      // 32 positions per workgroup
    if (p.family == DIRECT_KSPLIT) {
        kern = g.transposed ? ksplit_kernel<true>(p.nt, p.rd) : ksplit_kernel<false>(p.nt, p.rd);
        grid.z = g.transposed ? 8 : 1;
    } else if (p.family == DIRECT_GATHER) {
        kern = gather_kernel(p.nt, p.rd);
        grid.x = (unsigned)((a.total + 255) / 256);
    } else {
        kern = p.nt == 2 ? conv_direct_mfma_kernel<2, true> : conv_direct_mfma_kernel<1, true>;
    }
    hipLaunchKernelGGL(kern, grid, dim3(256), 0, st, a);
    return ru3d_check_launch(p.name);
}

}  // namespace RU3D_NS
