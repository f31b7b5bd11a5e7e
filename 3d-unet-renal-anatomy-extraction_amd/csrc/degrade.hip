// Image-quality augmentation of a sampled patch (ru3d_augment_degrade): Gaussian noise, Gaussian blur and simulated low
// resolution, the three ops of the usual 3D medical recipe that change sharpness, noise level and effective resolution.
// They sit between the resampling kernels of augment.hip and its intensity chain and act on the image only, on all
// channels of a patch [C][px][py][pz] with one parameter set.  The host draws the parameters (augment.py); the kernels
// are deterministic functions of (patch, parameters) and have numpy twins in degrade.py.
//
//   noise     Philox4x32-10, key (k0, k1), counter (j, 0, 0, 0): one call per four voxels (linear index i over the
//             whole patch, call j = i >> 2, normal i & 3), Box-Muller in float64, out = float32(x + sqrt(variance) * n)
//   blur      scipy.ndimage.gaussian_filter(sigma, mode='reflect', truncate=4) restated: radius r = int(4 sigma + 0.5),
//             weights normalised in float64 on the host, one pass per axis (x, y, z) through a ping-pong buffer; a pass
//             accumulates in float64 in scipy's order (centre, then the pairs from the outermost inwards) and stores
//             float32.  The z pass stages 64 + 2r voxels of a row per wave in LDS, the x / y passes a tile of
//             (16 + 2r) x 64 voxels: every source voxel is read from HBM once per pass (halo rows twice)
//   low-res   nearest-neighbour down to n_d = max(round(P_d * zoom), 2), order 1 back up, scipy.ndimage.zoom's
//             corner-aligned coordinates, fused into one gather of 8 nearest-sampled sources per output voxel; per-axis
//             tables {source index of the two low-grid neighbours, weight} are made once per launch by a one-block kernel
//   finish    moves the result back into the patch when the last op left it in the workspace and writes the per-block
//             {sum, min, max} partials in the layout and order of resample_kernel, for the intensity chain
//
// No atomics, no host synchronisation; every barrier sits in a loop whose bounds are uniform over the workgroup.
#include "common.h"
#include "bitvol.h"
#include <math.h>

namespace {

constexpr int MAX_R = RU3D_DEGRADE_MAX_RADIUS;
constexpr int BLUR_TILE = 16;                       // outputs along the filtered axis per tile of a strided pass

struct BlurWeights {
    double w[MAX_R + 1];                            // w[d]: the normalised weight at distance d from the centre
};

// ---------------------------------------------------------------------------------------------------------- noise
__device__ __forceinline__ void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int round = 0; round < 10; round++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
        c[0] = n0;
        c[1] = (uint32_t)p1;
        c[2] = n2;
        c[3] = (uint32_t)p0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}

__device__ __forceinline__ void box_muller(uint32_t a, uint32_t b, double& n0, double& n1) {
    const double ua = ((double)a + 0.5) * 0x1p-32, ub = ((double)b + 0.5) * 0x1p-32;
    const double radius = sqrt(-2.0 * log(ua));
    double s, c;
    sincos(6.283185307179586 * ub, &s, &c);
    n0 = radius * c;
    n1 = radius * s;
}

__global__ __launch_bounds__(256) void degrade_noise_kernel(float* __restrict__ img, int64_t count, double sd,
                                                            uint32_t k0, uint32_t k1) {
    const int64_t calls = (count + 3) >> 2;
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < calls; j += (int64_t)gridDim.x * 256) {
        uint32_t c[4] = {(uint32_t)j, (uint32_t)(j >> 32), 0u, 0u};
        philox4x32_10(c, k0, k1);
        double n[4];
        box_muller(c[0], c[1], n[0], n[1]);
        box_muller(c[2], c[3], n[2], n[3]);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int64_t i = 4 * j + k;
            if (i < count) img[i] = (float)((double)img[i] + sd * n[k]);
        }
    }
}

// ----------------------------------------------------------------------------------------------------------- blur
// scipy's reflect: ... b a | a b ...; one reflection is enough because r <= L (checked by the entry point).  Tile rows
// beyond L - 1 + r are never read by a live output; the clamp only keeps their address inside the line.
__device__ __forceinline__ int reflect(int q, int L) {
    q = q < 0 ? -q - 1 : (q >= L ? 2 * L - 1 - q : q);
    return q < 0 ? 0 : (q > L - 1 ? L - 1 : q);
}

__device__ __forceinline__ void stage_weights(double* w, const BlurWeights& bw) {
    if (threadIdx.x == 0) {
#pragma unroll
        for (int d = 0; d <= MAX_R; d++) w[d] = bw.w[d];
    }
}

// A pass along an axis that is not the contiguous one: element (o, l, i) of [outer][L][inner] at (o * L + l) * inner + i,
// filtered along l.  The x pass has inner = py * pz, the y pass inner = pz.  A tile is BLUR_TILE outputs along l by 64
// along i; lanes run along i (coalesced rows, conflict-free LDS columns), a wave takes every fourth row.
__global__ __launch_bounds__(256) void degrade_blur_strided_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                                   int L, int64_t inner, int r, BlurWeights bw,
                                                                   int64_t tiles, int ltiles, int64_t itiles) {
    __shared__ float tile[BLUR_TILE + 2 * MAX_R][64];
    __shared__ double w[MAX_R + 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    stage_weights(w, bw);
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t it = t % itiles, rest = t / itiles;
        const int l0 = (int)(rest % ltiles) * BLUR_TILE;
        const int64_t base = (rest / ltiles) * (int64_t)L * inner, i = it * 64 + lane;
        const bool in = i < inner;
        for (int k = wave; k < BLUR_TILE + 2 * r; k += 4)
            tile[k][lane] = in ? src[base + (int64_t)reflect(l0 - r + k, L) * inner + i] : 0.f;
        __syncthreads();
        for (int k = wave; k < BLUR_TILE; k += 4) {
            const int l = l0 + k;
            if (l < L && in) {
                double acc = (double)tile[k + r][lane] * w[0];
                for (int d = r; d >= 1; d--)
                    acc += ((double)tile[k + r - d][lane] + (double)tile[k + r + d][lane]) * w[d];
                dst[base + (int64_t)l * inner + i] = (float)acc;
            }
        }
        __syncthreads();                              // the next tile's staging overwrites what was just read
    }
}

// The pass along the contiguous axis: `rows` lines of L voxels.  A wave takes a line, 64 outputs at a time.
__global__ __launch_bounds__(256) void degrade_blur_rows_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                                int64_t rows, int L, int r, BlurWeights bw) {
    __shared__ float line[4][64 + 2 * MAX_R];
    __shared__ double w[MAX_R + 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    stage_weights(w, bw);
    const int chunks = (L + 63) / 64;
    for (int64_t row0 = (int64_t)blockIdx.x * 4; row0 < rows; row0 += (int64_t)gridDim.x * 4) {
        const int64_t row = row0 + wave;
        const bool live = row < rows;
        for (int ch = 0; ch < chunks; ch++) {
            const int z0 = ch * 64;
            for (int t = lane; t < 64 + 2 * r; t += 64)
                line[wave][t] = live ? src[row * L + reflect(z0 - r + t, L)] : 0.f;
            __syncthreads();
            const int z = z0 + lane;
            if (live && z < L) {
                double acc = (double)line[wave][lane + r] * w[0];
                for (int d = r; d >= 1; d--)
                    acc += ((double)line[wave][lane + r - d] + (double)line[wave][lane + r + d]) * w[d];
                dst[row * L + z] = (float)acc;
            }
            __syncthreads();
        }
    }
}

// -------------------------------------------------------------------------------------------------------- low-res
struct LowResTap {
    int32_t s0, s1;                                 // source voxels of the low-grid neighbours floor(t), floor(t) + 1
    double w;                                       // t - floor(t)
};

struct LowResAxes {
    int P[3], n[3];
    double up[3], down[3];                          // (n - 1) / (P - 1) and (P - 1) / (n - 1), formed once in float64
};

__global__ __launch_bounds__(256) void degrade_lowres_tables_kernel(LowResTap* __restrict__ tab, LowResAxes ax) {
    int off = 0;
#pragma unroll
    for (int d = 0; d < 3; d++) {
        const int P = ax.P[d], n = ax.n[d];
        for (int o = threadIdx.x; o < P; o += 256) {
            const double t = (double)o * ax.up[d], f = floor(t);
            int l0 = (int)f;
            l0 = l0 < 0 ? 0 : (l0 > n - 1 ? n - 1 : l0);
            const int l1 = l0 + 1 > n - 1 ? n - 1 : l0 + 1;     // beyond the low grid: scipy's reflect reads the last one
            int s0 = (int)floor((double)l0 * ax.down[d] + 0.5), s1 = (int)floor((double)l1 * ax.down[d] + 0.5);
            LowResTap tap;
            tap.s0 = s0 < 0 ? 0 : (s0 > P - 1 ? P - 1 : s0);
            tap.s1 = s1 < 0 ? 0 : (s1 > P - 1 ? P - 1 : s1);
            tap.w = t - f;
            tab[off + o] = tap;
        }
        off += P;
    }
}

// scipy's order: the 8 neighbours with the last axis fastest, each value times its three weights in turn, summed as they
// come; products and sums are kept apart (no fused multiply-add) so that the float64 sum is scipy's to the bit
__device__ __forceinline__ float lowres_sum(const float (&v)[8], const double (&wx)[2], const double (&wy)[2],
                                            const double (&wz)[2]) {
#pragma clang fp contract(off)
    double t = 0.0;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        double coeff = (double)v[k];
        coeff *= wx[k >> 2];
        coeff *= wy[(k >> 1) & 1];
        coeff *= wz[k & 1];
        t += coeff;
    }
    return (float)t;
}

__global__ __launch_bounds__(256) void degrade_lowres_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                             int C, int px, int py, int pz,
                                                             const LowResTap* __restrict__ tab) {
    const int64_t total = (int64_t)px * py * pz;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int oz = (int)(i % pz);
    const int64_t rest = i / pz;
    const LowResTap tx = tab[(int)(rest / py)], ty = tab[px + (int)(rest % py)], tz = tab[px + py + oz];
    const int64_t xs[2] = {(int64_t)tx.s0 * py * pz, (int64_t)tx.s1 * py * pz};
    const int64_t ys[2] = {(int64_t)ty.s0 * pz, (int64_t)ty.s1 * pz};
    const int64_t zs[2] = {tz.s0, tz.s1};
    const double wx[2] = {1.0 - tx.w, tx.w}, wy[2] = {1.0 - ty.w, ty.w}, wz[2] = {1.0 - tz.w, tz.w};
    for (int c = 0; c < C; c++) {
        const float* s = src + (int64_t)c * total;
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; k++) v[k] = s[xs[k >> 2] + ys[(k >> 1) & 1] + zs[k & 1]];
        dst[(int64_t)c * total + i] = lowres_sum(v, wx, wy, wz);
    }
}

// --------------------------------------------------------------------------------------------------------- finish
// Block b takes voxels 256 b .. 256 b + 255 of every channel: the partials of resample_kernel, in its order.
__global__ __launch_bounds__(256) void degrade_finish_kernel(const float* src, float* dst,
                                                             int C, int64_t total, double* __restrict__ part) {
    __shared__ double red[3][4];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double s = 0.0;
    float mn = INFINITY, mx = -INFINITY;
    if (i < total) {
        for (int c = 0; c < C; c++) {
            const float v = src[(int64_t)c * total + i];
            if (dst != src) dst[(int64_t)c * total + i] = v;
            s += (double)v;
            mn = fminf(mn, v);
            mx = fmaxf(mx, v);
        }
    }
    double ws = s;
    float wmn = mn, wmx = mx;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        ws += __shfl_xor(ws, o, 64);
        wmn = fminf(wmn, __shfl_xor(wmn, o, 64));
        wmx = fmaxf(wmx, __shfl_xor(wmx, o, 64));
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        red[0][wave] = ws;
        red[1][wave] = (double)wmn;
        red[2][wave] = (double)wmx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0, a = red[1][0], b = red[2][0];
        for (int k = 0; k < 4; k++) {
            t += red[0][k];
            a = fmin(a, red[1][k]);
            b = fmax(b, red[2][k]);
        }
        part[3 * blockIdx.x] = t;
        part[3 * blockIdx.x + 1] = a;
        part[3 * blockIdx.x + 2] = b;
    }
}

int blur_radius(double sigma) { return (int)(4.0 * sigma + 0.5); }

}  // namespace

extern "C" size_t ru3d_augment_degrade_workspace_bytes(int C, int px, int py, int pz) {
    if (C <= 0 || px <= 0 || py <= 0 || pz <= 0) return 0;
    const size_t total = (size_t)px * py * pz;
    return bv_align(total * C * sizeof(float)) + bv_align(((size_t)px + py + pz) * sizeof(LowResTap)) + 256;
}

extern "C" int ru3d_augment_degrade(float* image, int C, int px, int py, int pz, const ru3d_degrade_params* p, void* ws,
                                    size_t ws_bytes, double* part, void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    RU3D_REQUIRE(image && p && ws && part && C > 0, "augment_degrade: bad argument");
    RU3D_REQUIRE(px > 0 && py > 0 && pz > 0, "augment_degrade: empty patch");
    const int64_t total = (int64_t)px * py * pz;
    RU3D_REQUIRE(total < (1ll << 31) && total * C < (1ll << 34), "augment_degrade: patch too large");
    RU3D_REQUIRE(ws_bytes >= ru3d_augment_degrade_workspace_bytes(C, px, py, pz), "augment_degrade: workspace too small");
    const int smallest = px < py ? (px < pz ? px : pz) : (py < pz ? py : pz);
    int r = 0;
    if (p->do_noise)
        RU3D_REQUIRE(isfinite(p->noise_variance) && p->noise_variance >= 0.0,
                     "augment_degrade: noise_variance %g is not a finite non-negative number", p->noise_variance);
    if (p->do_blur) {
        RU3D_REQUIRE(isfinite(p->blur_sigma) && p->blur_sigma > 0.0, "augment_degrade: blur_sigma %g is not positive",
                     p->blur_sigma);
        RU3D_REQUIRE(p->blur_sigma < 1e6 && blur_radius(p->blur_sigma) <= RU3D_DEGRADE_MAX_RADIUS,
                     "augment_degrade: blur_sigma %g gives a radius above %d", p->blur_sigma, RU3D_DEGRADE_MAX_RADIUS);
        r = blur_radius(p->blur_sigma);
        RU3D_REQUIRE(r <= smallest, "augment_degrade: blur radius %d exceeds the smallest patch extent %d", r, smallest);
    }
    if (p->do_low_res) {
        RU3D_REQUIRE(p->low_res_zoom > 0.0 && p->low_res_zoom <= 1.0, "augment_degrade: low_res_zoom %g is outside (0, 1]",
                     p->low_res_zoom);
        RU3D_REQUIRE(smallest >= 2, "augment_degrade: low resolution needs at least 2 voxels per axis");
    }
    const hipStream_t st = as_stream(stream);
    const int64_t count = total * C;
    float* other = (float*)ws;
    LowResTap* tab = (LowResTap*)((char*)ws + bv_align((size_t)count * sizeof(float)));
    float* cur = image;
    if (p->do_noise) {
        const int64_t calls = (count + 3) >> 2;
        int64_t blocks = (calls + 255) / 256;
        if (blocks > 8192) blocks = 8192;
        hipLaunchKernelGGL(degrade_noise_kernel, dim3((unsigned)blocks), dim3(256), 0, st, image, count,
                           sqrt(p->noise_variance), p->noise_key[0], p->noise_key[1]);
        int rc = ru3d_check_launch("augment_degrade_noise");
        if (rc) return rc;
    }
    if (p->do_blur) {
        BlurWeights bw;
        const double scale = -0.5 / (p->blur_sigma * p->blur_sigma);
        double sum = 0.0;
        for (int d = -r; d <= r; d++) sum += exp(scale * (double)(d * d));
        for (int d = 0; d <= MAX_R; d++) bw.w[d] = d <= r ? exp(scale * (double)(d * d)) / sum : 0.0;
        // x: image -> workspace, y: workspace -> image, z: image -> workspace
        const int L[2] = {px, py};
        const int64_t inner[2] = {(int64_t)py * pz, (int64_t)pz}, outer[2] = {C, (int64_t)C * px};
        for (int a = 0; a < 2; a++) {
            const int ltiles = (L[a] + BLUR_TILE - 1) / BLUR_TILE;
            const int64_t itiles = (inner[a] + 63) / 64, tiles = outer[a] * ltiles * itiles;
            const int64_t blocks = tiles < 8192 ? tiles : 8192;
            hipLaunchKernelGGL(degrade_blur_strided_kernel, dim3((unsigned)blocks), dim3(256), 0, st,
                               a == 0 ? image : other, a == 0 ? other : image, L[a], inner[a], r, bw, tiles, ltiles,
                               itiles);
            int rc = ru3d_check_launch("augment_degrade_blur");
            if (rc) return rc;
        }
        const int64_t rows = (int64_t)C * px * py;
        int64_t blocks = (rows + 3) / 4;
        if (blocks > 8192) blocks = 8192;
        hipLaunchKernelGGL(degrade_blur_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, st, image, other, rows, pz, r, bw);
        int rc = ru3d_check_launch("augment_degrade_blur_rows");
        if (rc) return rc;
        cur = other;
    }
    const unsigned vblocks = (unsigned)((total + 255) / 256);
    if (p->do_low_res) {
        LowResAxes ax;
        const int P[3] = {px, py, pz};
        for (int d = 0; d < 3; d++) {
            int n = (int)nearbyint((double)P[d] * p->low_res_zoom);          // np.round: halves to even
            n = n < 2 ? 2 : n;
            ax.P[d] = P[d];
            ax.n[d] = n;
            ax.up[d] = (double)(n - 1) / (double)(P[d] - 1);
            ax.down[d] = (double)(P[d] - 1) / (double)(n - 1);
        }
        hipLaunchKernelGGL(degrade_lowres_tables_kernel, dim3(1), dim3(256), 0, st, tab, ax);
        int rc = ru3d_check_launch("augment_degrade_lowres_tables");
        if (rc) return rc;
        float* to = cur == image ? other : image;
        hipLaunchKernelGGL(degrade_lowres_kernel, dim3(vblocks), dim3(256), 0, st, cur, to, C, px, py, pz, tab);
        rc = ru3d_check_launch("augment_degrade_lowres");
        if (rc) return rc;
        cur = to;
    }
    hipLaunchKernelGGL(degrade_finish_kernel, dim3(vblocks), dim3(256), 0, st, cur, image, C, total, part);
    return ru3d_check_launch("augment_degrade_finish");
}
