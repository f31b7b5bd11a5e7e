// On-device patch sampling + augmentation: the reference's training transform chain
//   RandomRescaleCrop -> RandomMirror -> RandomContrast -> RandomBrightness -> RandomGamma -> ToTensor
// (transform.py:573-652, 279-301, 176-259, 156-163; composed in nb_train_iia.py:30-39) as three small HBM-bound
// kernels per patch.  The random draws are made by the host in the reference's order (augment.py); the kernels are
// deterministic functions of (volume, parameters), so a patch can be replayed against the CPU pipeline.
//
//   presence   which label values occur in the crop box (decides the label resampling rule, transform.py:47-48, and
//              serves enforce_label_indices, :620-637)
//   resample   crop + constant pad + scipy.ndimage.zoom(order=1) restated: output sample o of an axis reads crop
//              coordinate o * (before - 1) / (patch - 1), trilinear interpolation in float64, float32 result;
//              labels: < 3 classes present: interpolate the label and truncate (transform.py:60-65), else one-hot per
//              class, interpolate, first maximum (:66-74); the mirror is folded into the output index; per-block
//              {sum, min, max} of the image for the intensity ops
//   intensity  contrast about the mean, brightness about the minimum, gamma on the [min, max] range, float32
//              arithmetic in the reference's order of operations; the minima / maxima after each monotone step are
//              derived from the resampled image's own, so one reduction serves all three ops
//   spatial    resample's free-form sibling (ru3d_augment_patch_spatial): the source coordinate of an output voxel is
//              centre + matrix . (u + D), u the centred patch index, D a cubic B-spline displacement from a small control
//              lattice; the 8 neighbours are gathered from the volume itself (outside = the pad constant); interpolation,
//              label rule and partials as resample
#include "common.h"
#include <math.h>

namespace {

struct Axis {
    double step;      // crop coordinate per output sample
    int before, lo, ext, patch, flip;
};

__device__ __forceinline__ void axis_sample(const Axis& a, int o, int& i0, int& i1, double& w) {
    const int s = a.flip ? a.patch - 1 - o : o;
    const double c = (double)s * a.step;
    int f = (int)floor(c);
    f = f < 0 ? 0 : (f > a.before - 1 ? a.before - 1 : f);
    w = c - (double)f;
    i0 = f;
    i1 = f + 1 > a.before - 1 ? a.before - 1 : f + 1;
}

template <typename L>
__device__ __forceinline__ int load_label(const L* lab, int64_t idx) { return (int)lab[idx]; }

template <typename L>
__global__ __launch_bounds__(256) void presence_kernel(const L* __restrict__ label, int X, int Y, int Z, int lx, int ly,
                                                       int lz, int bx, int by, int bz, int cval,
                                                       unsigned* __restrict__ mask) {
    const int64_t total = (int64_t)bx * by * bz;
    unsigned m = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int z = (int)(i % bz);
        const int64_t t = i / bz;
        const int y = (int)(t % by), x = (int)(t / by);
        const int gx = lx + x, gy = ly + y, gz = lz + z;
        int v = cval;
        if (gx >= 0 && gx < X && gy >= 0 && gy < Y && gz >= 0 && gz < Z) v = load_label(label, ((int64_t)gx * Y + gy) * Z + gz);
        m |= 1u << (v < 0 ? 0 : (v > 31 ? 31 : v));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m |= __shfl_xor((int)m, o, 64);
    if ((threadIdx.x & 63) == 0 && m) atomicOr(mask, m);
}

template <typename L>
__global__ __launch_bounds__(256) void resample_kernel(const float* __restrict__ image, const L* __restrict__ label,
                                                       int X, int Y, int Z, int C, Axis ax, Axis ay, Axis az,
                                                       float image_cval, int label_cval,
                                                       const unsigned* __restrict__ mask, float* __restrict__ out_image,
                                                       int64_t* __restrict__ out_label, double* __restrict__ part) {
    __shared__ double red[3][4];
    const int64_t total = (int64_t)ax.patch * ay.patch * az.patch;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double s = 0.0;
    float mn = INFINITY, mx = -INFINITY;
    if (i < total) {
        const int oz = (int)(i % az.patch);
        const int64_t t = i / az.patch;
        const int oy = (int)(t % ay.patch), ox = (int)(t / ay.patch);
        int x0, x1, y0, y1, z0, z1;
        double wx, wy, wz;
        axis_sample(ax, ox, x0, x1, wx);
        axis_sample(ay, oy, y0, y1, wy);
        axis_sample(az, oz, z0, z1, wz);
        const int xs[2] = {ax.lo + x0, ax.lo + x1}, ys[2] = {ay.lo + y0, ay.lo + y1}, zs[2] = {az.lo + z0, az.lo + z1};
        const double wxs[2] = {1.0 - wx, wx}, wys[2] = {1.0 - wy, wy}, wzs[2] = {1.0 - wz, wz};
        int64_t src[8];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int gx = xs[k >> 2], gy = ys[(k >> 1) & 1], gz = zs[k & 1];
            const bool in = gx >= 0 && gx < X && gy >= 0 && gy < Y && gz >= 0 && gz < Z;
            src[k] = in ? ((int64_t)gx * Y + gy) * Z + gz : -1;
        }
        // separable order of scipy's zoom: axis 0 first, then 1, then 2 (each a float64 lerp)
        for (int c = 0; image && c < C; c++) {
            double v[8];
#pragma unroll
            for (int k = 0; k < 8; k++) v[k] = src[k] >= 0 ? (double)image[src[k] * C + c] : (double)image_cval;
            double a4[4];
#pragma unroll
            for (int k = 0; k < 4; k++) a4[k] = v[k] * wxs[0] + v[k + 4] * wxs[1];
            const double b0 = a4[0] * wys[0] + a4[2] * wys[1], b1 = a4[1] * wys[0] + a4[3] * wys[1];
            const float r = (float)(b0 * wzs[0] + b1 * wzs[1]);
            out_image[(int64_t)c * total + i] = r;
            s += (double)r;
            mn = fminf(mn, r);
            mx = fmaxf(mx, r);
        }
        if (label && out_label) {
            int lv[8];
#pragma unroll
            for (int k = 0; k < 8; k++) lv[k] = src[k] >= 0 ? load_label(label, src[k]) : label_cval;
            const unsigned m = mask ? *mask : 0xffffffffu;
            const int num_classes = 32 - __clz((int)m);          // highest label present + 1
            int64_t res;
            if (num_classes < 3) {
                double a4[4];
#pragma unroll
                for (int k = 0; k < 4; k++) a4[k] = (double)lv[k] * wxs[0] + (double)lv[k + 4] * wxs[1];
                const double b0 = a4[0] * wys[0] + a4[2] * wys[1], b1 = a4[1] * wys[0] + a4[3] * wys[1];
                const float r = (float)(b0 * wzs[0] + b1 * wzs[1]);
                res = (int64_t)r;                                  // astype(integer dtype): truncation
            } else {
                int best = 0x7fffffff;
                float best_w = -1.f;
#pragma unroll
                for (int k = 0; k < 8; k++) {
                    // the class plane's interpolated value, in the separable order used for images
                    double v[8];
#pragma unroll
                    for (int j = 0; j < 8; j++) v[j] = lv[j] == lv[k] ? 1.0 : 0.0;
                    double a4[4];
#pragma unroll
                    for (int j = 0; j < 4; j++) a4[j] = v[j] * wxs[0] + v[j + 4] * wxs[1];
                    const double b0 = a4[0] * wys[0] + a4[2] * wys[1], b1 = a4[1] * wys[0] + a4[3] * wys[1];
                    const float tw = (float)(b0 * wzs[0] + b1 * wzs[1]);
                    if (tw > best_w || (tw == best_w && lv[k] < best)) {
                        best_w = tw;
                        best = lv[k];
                    }
                }
                // classes that are not among the 8 neighbours have plane value 0 and the maximum is positive (the
                // weights sum to one), so the first maximum over all classes is the best neighbour class
                res = best;
            }
            out_label[i] = res;
        }
    }
    // block partials: fixed order
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

__global__ __launch_bounds__(256) void intensity_kernel(float* __restrict__ img, int64_t count,
                                                        const double* __restrict__ part, int nparts, int do_contrast,
                                                        float fc, int do_brightness, float fb, int do_gamma, float fg,
                                                        float eps) {
    __shared__ double red[3][256];
    double s = 0.0, a = INFINITY, b = -INFINITY;
    for (int k = threadIdx.x; k < nparts; k += 256) {
        s += part[3 * k];
        a = fmin(a, part[3 * k + 1]);
        b = fmax(b, part[3 * k + 2]);
    }
    red[0][threadIdx.x] = s;
    red[1][threadIdx.x] = a;
    red[2][threadIdx.x] = b;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            red[0][threadIdx.x] += red[0][threadIdx.x + o];
            red[1][threadIdx.x] = fmin(red[1][threadIdx.x], red[1][threadIdx.x + o]);
            red[2][threadIdx.x] = fmax(red[2][threadIdx.x], red[2][threadIdx.x + o]);
        }
        __syncthreads();
    }
    const float mean = (float)(red[0][0] / (double)count);
    float mn = (float)red[1][0], mx = (float)red[2][0];
    // every step below is monotone in the voxel value (also after float32 rounding), so the extrema follow the extrema
    auto contrast = [&](float v) { return (v - mean) * fc + mean; };
    float mn1 = mn, mx1 = mx;
    if (do_contrast) {
        const float lo = contrast(mn), hi = contrast(mx);
        mn1 = fminf(lo, hi);
        mx1 = fmaxf(lo, hi);
    }
    auto bright = [&](float v) { return (v - mn1) * fb + mn1; };
    float mn2 = mn1, mx2 = mx1;
    if (do_brightness) {
        const float lo = bright(mn1), hi = bright(mx1);
        mn2 = fminf(lo, hi);
        mx2 = fmaxf(lo, hi);
    }
    const float arange = mx2 - mn2 + eps;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 256) {
        float v = img[i];
        if (do_contrast) v = contrast(v);
        if (do_brightness) v = bright(v);
        if (do_gamma) v = powf((v - mn2) / arange, fg) * arange + mn2;
        img[i] = v;
    }
}

// ---------------------------------------------------------------------------------------------- spatial transform
// Work is cut into groups of SPATIAL_ROWS output rows (runs along z) that share ox; a workgroup takes groups
// blockIdx.x, + gridDim.x, ...  Along a row the x and y lattice cells and weights are uniform, so the 4 x 4 x 4 control
// points of a voxel are collapsed in three steps: x once per group into `slab` (all threads), y once per row into the
// wave's `row`, z per voxel (4 x 3 multiply-adds).  Every loop bound and barrier below is uniform over the workgroup.
constexpr int SPATIAL_ROWS = 8;

struct Spatial {
    double c[3], m[9];
    int patch[3], flip[3], n[3], g[3];
    int elastic, ychunks, groups;
};

__device__ __forceinline__ void bspline_weights(double f, double (&b)[4]) {
    const double sixth = 1.0 / 6.0, e = 1.0 - f, f2 = f * f, f3 = f2 * f;
    b[0] = e * e * e * sixth;
    b[1] = (3.0 * f3 - 6.0 * f2 + 4.0) * sixth;
    b[2] = (-3.0 * f3 + 3.0 * f2 + 3.0 * f + 1.0) * sixth;
    b[3] = f3 * sixth;
}

// lattice cell and weights of (mirrored) patch index o.  i <= n - 3: tap i + 3 lies beyond the lattice exactly where
// (P - 1) / g is whole and o is the last voxel, with weight B_3(0) = 0; lattice_tap() sends it to the last point.
__device__ __forceinline__ void lattice_cell(int o, int g, int n, int& i, double (&b)[4]) {
    const double t = (double)o / (double)g;
    i = (int)t;
    i = i > n - 1 ? n - 1 : i;
    bspline_weights(t - (double)i, b);
}
__device__ __forceinline__ int lattice_tap(int i, int a, int n) { return i + a < n ? i + a : n - 1; }

__device__ __forceinline__ void source_axis(double s, int ext, int& i0, double& w) {
    s = fmin(fmax(s, -2.0), (double)ext + 1.0);       // also takes a NaN to -2: every neighbour outside
    const double f = floor(s);
    i0 = (int)f;
    w = s - f;
}

// float64 lerps along axis 0, then 1, then 2 (neighbour k = 4 * dx + 2 * dy + dz), rounded to float32
__device__ __forceinline__ float trilerp(const double (&v)[8], const double (&wx)[2], const double (&wy)[2],
                                         const double (&wz)[2]) {
    double a4[4];
#pragma unroll
    for (int k = 0; k < 4; k++) a4[k] = v[k] * wx[0] + v[k + 4] * wx[1];
    const double b0 = a4[0] * wy[0] + a4[2] * wy[1], b1 = a4[1] * wy[0] + a4[3] * wy[1];
    return (float)(b0 * wz[0] + b1 * wz[1]);
}

template <typename L>
__global__ __launch_bounds__(256) void spatial_kernel(const float* __restrict__ image, const L* __restrict__ label,
                                                      int X, int Y, int Z, int C, Spatial sp, float image_cval,
                                                      int label_cval, const float* __restrict__ lattice,
                                                      const unsigned* __restrict__ mask, float* __restrict__ out_image,
                                                      int64_t* __restrict__ out_label, double* __restrict__ part) {
    extern __shared__ double spatial_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int px = sp.patch[0], py = sp.patch[1], pz = sp.patch[2];
    const int nx = sp.n[0], ny = sp.n[1], nz = sp.n[2], nyz = ny * nz;
    double* red = spatial_lds;                        // [3][4]
    double* slab = spatial_lds + 12;                  // [3][ny][nz]: the lattice collapsed along x
    double* row = slab + 3 * nyz + wave * 3 * nz;     // [3][nz] per wave: collapsed along x and y
    const int64_t total = (int64_t)px * py * pz;
    const unsigned present = mask ? *mask : 0xffffffffu;
    const int num_classes = 32 - __clz((int)present);            // highest label present + 1
    double s = 0.0;
    float mn = INFINITY, mx = -INFINITY;
    for (int grp = blockIdx.x; grp < sp.groups; grp += gridDim.x) {
        const int ox = grp / sp.ychunks, y0 = (grp - ox * sp.ychunks) * SPATIAL_ROWS;
        const int fx = sp.flip[0] ? px - 1 - ox : ox;
        const double ux = (double)fx - 0.5 * (double)(px - 1);
        if (sp.elastic) {
            int ix;
            double bx[4];
            lattice_cell(fx, sp.g[0], nx, ix, bx);
            __syncthreads();                          // the previous group's rows no longer read the slab
            for (int idx = threadIdx.x; idx < 3 * nyz; idx += 256) {
                const int k = idx / nyz, r = idx - k * nyz;
                const float* src = lattice + (int64_t)k * nx * nyz + r;
                double v = 0.0;
#pragma unroll
                for (int a = 0; a < 4; a++) v += bx[a] * (double)src[(int64_t)lattice_tap(ix, a, nx) * nyz];
                slab[idx] = v;
            }
            __syncthreads();
        }
        for (int r = wave; r < SPATIAL_ROWS; r += 4) {
            const int oy = y0 + r;
            const bool live = oy < py;
            const int fy = live ? (sp.flip[1] ? py - 1 - oy : oy) : 0;
            const double uy = (double)fy - 0.5 * (double)(py - 1);
            if (sp.elastic) {
                int iy;
                double by[4];
                lattice_cell(fy, sp.g[1], ny, iy, by);
                for (int idx = lane; live && idx < 3 * nz; idx += 64) {
                    const int k = idx / nz, j = idx - k * nz;
                    const double* src = slab + k * nyz + j;
                    double v = 0.0;
#pragma unroll
                    for (int b = 0; b < 4; b++) v += by[b] * src[lattice_tap(iy, b, ny) * nz];
                    row[idx] = v;
                }
                __syncthreads();                      // the row is read by other lanes than the ones that wrote it
            }
            for (int oz = lane; live && oz < pz; oz += 64) {
                const int fz = sp.flip[2] ? pz - 1 - oz : oz;
                double q[3] = {ux, uy, (double)fz - 0.5 * (double)(pz - 1)};
                if (sp.elastic) {
                    int iz;
                    double bz[4];
                    lattice_cell(fz, sp.g[2], nz, iz, bz);
#pragma unroll
                    for (int k = 0; k < 3; k++) {
                        double d = 0.0;
#pragma unroll
                        for (int c = 0; c < 4; c++) d += bz[c] * row[k * nz + lattice_tap(iz, c, nz)];
                        q[k] += d;
                    }
                }
                int i0[3];
                double w[3];
                source_axis(sp.c[0] + (sp.m[0] * q[0] + sp.m[1] * q[1] + sp.m[2] * q[2]), X, i0[0], w[0]);
                source_axis(sp.c[1] + (sp.m[3] * q[0] + sp.m[4] * q[1] + sp.m[5] * q[2]), Y, i0[1], w[1]);
                source_axis(sp.c[2] + (sp.m[6] * q[0] + sp.m[7] * q[1] + sp.m[8] * q[2]), Z, i0[2], w[2]);
                const double wxs[2] = {1.0 - w[0], w[0]}, wys[2] = {1.0 - w[1], w[1]}, wzs[2] = {1.0 - w[2], w[2]};
                int64_t src[8];
#pragma unroll
                for (int k = 0; k < 8; k++) {
                    const int gx = i0[0] + (k >> 2), gy = i0[1] + ((k >> 1) & 1), gz = i0[2] + (k & 1);
                    const bool in = gx >= 0 && gx < X && gy >= 0 && gy < Y && gz >= 0 && gz < Z;
                    src[k] = in ? ((int64_t)gx * Y + gy) * Z + gz : -1;
                }
                const int64_t i = ((int64_t)ox * py + oy) * pz + oz;
                for (int c = 0; image && c < C; c++) {
                    double v[8];
#pragma unroll
                    for (int k = 0; k < 8; k++) v[k] = src[k] >= 0 ? (double)image[src[k] * C + c] : (double)image_cval;
                    const float r32 = trilerp(v, wxs, wys, wzs);
                    out_image[(int64_t)c * total + i] = r32;
                    s += (double)r32;
                    mn = fminf(mn, r32);
                    mx = fmaxf(mx, r32);
                }
                if (label && out_label) {
                    int lv[8];
#pragma unroll
                    for (int k = 0; k < 8; k++) lv[k] = src[k] >= 0 ? load_label(label, src[k]) : label_cval;
                    double v[8];
                    int64_t res;
                    if (num_classes < 3) {
#pragma unroll
                        for (int k = 0; k < 8; k++) v[k] = (double)lv[k];
                        res = (int64_t)trilerp(v, wxs, wys, wzs);            // astype(integer dtype): truncation
                    } else {
                        // as resample_kernel: the neighbour class with the largest interpolated one-hot plane value,
                        // the smallest class on ties
                        int best = 0x7fffffff;
                        float best_w = -1.f;
#pragma unroll
                        for (int k = 0; k < 8; k++) {
#pragma unroll
                            for (int j = 0; j < 8; j++) v[j] = lv[j] == lv[k] ? 1.0 : 0.0;
                            const float tw = trilerp(v, wxs, wys, wzs);
                            if (tw > best_w || (tw == best_w && lv[k] < best)) {
                                best_w = tw;
                                best = lv[k];
                            }
                        }
                        res = best;
                    }
                    out_label[i] = res;
                }
            }
        }
    }
    // block partials: fixed order (a thread's voxels in loop order, the wave by shuffles, the four waves in turn)
    double ws = s;
    float wmn = mn, wmx = mx;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        ws += __shfl_xor(ws, o, 64);
        wmn = fminf(wmn, __shfl_xor(wmn, o, 64));
        wmx = fmaxf(wmx, __shfl_xor(wmx, o, 64));
    }
    if (lane == 0) {
        red[wave] = ws;
        red[4 + wave] = (double)wmn;
        red[8 + wave] = (double)wmx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0, a = red[4], b = red[8];
        for (int k = 0; k < 4; k++) {
            t += red[k];
            a = fmin(a, red[4 + k]);
            b = fmax(b, red[8 + k]);
        }
        part[3 * blockIdx.x] = t;
        part[3 * blockIdx.x + 1] = a;
        part[3 * blockIdx.x + 2] = b;
    }
}

Axis make_axis(int lo, int before, int ext, int patch, int flip) {
    Axis a;
    a.lo = lo; a.before = before; a.ext = ext; a.patch = patch; a.flip = flip;
    a.step = patch > 1 ? (double)(before - 1) / (double)(patch - 1) : 0.0;
    return a;
}

// the intensity chain behind either resampling kernel, fed by its `nparts` per-block partials
int launch_intensity(bool have_image, const ru3d_patch_params* p, float* out_image, int64_t count, const double* part,
                     int nparts, void* stream) {
    if (!have_image || !(p->do_contrast || p->do_brightness || p->do_gamma)) return 0;
    int64_t ib = (count + 1023) / 1024;
    if (ib > 512) ib = 512;
    hipLaunchKernelGGL(intensity_kernel, dim3((unsigned)ib), dim3(256), 0, as_stream(stream), out_image, count, part,
                       nparts, p->do_contrast, p->contrast, p->do_brightness, p->brightness, p->do_gamma, p->gamma,
                       p->gamma_eps);
    return ru3d_check_launch("augment_intensity");
}

}  // namespace

extern "C" size_t ru3d_augment_workspace_bytes(int px, int py, int pz) {
    if (px <= 0 || py <= 0 || pz <= 0) return 0;
    const int64_t total = (int64_t)px * py * pz;
    return (size_t)((total + 255) / 256) * 3 * sizeof(double) + 256;
}

extern "C" int ru3d_augment_label_presence(const void* label, int label_dtype, int X, int Y, int Z, const int32_t* lo,
                                           const int32_t* before, int label_cval, uint32_t* mask, void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    RU3D_REQUIRE(label && lo && before && mask && X > 0 && Y > 0 && Z > 0, "augment_label_presence: bad argument");
    RU3D_REQUIRE(before[0] > 0 && before[1] > 0 && before[2] > 0, "augment_label_presence: empty crop box");
    hipError_t e = hipMemsetAsync(mask, 0, sizeof(uint32_t), as_stream(stream));
    if (e != hipSuccess) return ru3d_fail((int)e, "augment_label_presence: memset: %s", hipGetErrorString(e));
    const int64_t total = (int64_t)before[0] * before[1] * before[2];
    int64_t blocks = (total + 1023) / 1024;
    if (blocks > 1024) blocks = 1024;
    if (label_dtype == RU3D_LABEL_U8)
        hipLaunchKernelGGL(presence_kernel<uint8_t>, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream),
                           (const uint8_t*)label, X, Y, Z, lo[0], lo[1], lo[2], before[0], before[1], before[2],
                           label_cval, mask);
    else if (label_dtype == RU3D_LABEL_I64)
        hipLaunchKernelGGL(presence_kernel<int64_t>, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream),
                           (const int64_t*)label, X, Y, Z, lo[0], lo[1], lo[2], before[0], before[1], before[2],
                           label_cval, mask);
    else
        return ru3d_fail(-1, "augment_label_presence: bad label dtype %d", label_dtype);
    return ru3d_check_launch("augment_label_presence");
}

extern "C" int ru3d_augment_patch(const float* image, const void* label, int label_dtype, int X, int Y, int Z, int C,
                                  const ru3d_patch_params* p, const uint32_t* presence_mask, float* out_image,
                                  int64_t* out_label, void* ws, size_t ws_bytes, void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    RU3D_REQUIRE(p && ws && X > 0 && Y > 0 && Z > 0 && C > 0, "augment_patch: bad argument");
    RU3D_REQUIRE((image == nullptr) == (out_image == nullptr), "augment_patch: image and out_image go together");
    RU3D_REQUIRE((label == nullptr) == (out_label == nullptr), "augment_patch: label and out_label go together");
    RU3D_REQUIRE(image || label, "augment_patch: nothing to resample");
    for (int d = 0; d < 3; d++)
        RU3D_REQUIRE(p->before[d] > 0 && p->patch[d] > 0, "augment_patch: empty crop box / patch on axis %d", d);
    RU3D_REQUIRE(ws_bytes >= ru3d_augment_workspace_bytes(p->patch[0], p->patch[1], p->patch[2]),
                 "augment_patch: workspace too small");
    RU3D_REQUIRE((int64_t)X * Y * Z * C < (1ll << 40), "augment_patch: volume too large");
    const int64_t total = (int64_t)p->patch[0] * p->patch[1] * p->patch[2];
    RU3D_REQUIRE(total < (1ll << 31), "augment_patch: patch too large");
    const Axis ax = make_axis(p->lo[0], p->before[0], X, p->patch[0], p->flip[0]);
    const Axis ay = make_axis(p->lo[1], p->before[1], Y, p->patch[1], p->flip[1]);
    const Axis az = make_axis(p->lo[2], p->before[2], Z, p->patch[2], p->flip[2]);
    const unsigned blocks = (unsigned)((total + 255) / 256);
    double* part = (double*)ws;
    if (!label || label_dtype == RU3D_LABEL_U8)
        hipLaunchKernelGGL(resample_kernel<uint8_t>, dim3(blocks), dim3(256), 0, as_stream(stream), image,
                           (const uint8_t*)label, X, Y, Z, C, ax, ay, az, p->image_cval, p->label_cval, presence_mask,
                           out_image, out_label, part);
    else if (label_dtype == RU3D_LABEL_I64)
        hipLaunchKernelGGL(resample_kernel<int64_t>, dim3(blocks), dim3(256), 0, as_stream(stream), image,
                           (const int64_t*)label, X, Y, Z, C, ax, ay, az, p->image_cval, p->label_cval, presence_mask,
                           out_image, out_label, part);
    else
        return ru3d_fail(-1, "augment_patch: bad label dtype %d", label_dtype);
    int rc = ru3d_check_launch("augment_resample");
    if (rc) return rc;
    return launch_intensity(image != nullptr, p, out_image, total * C, part, (int)blocks, stream);
}

extern "C" int ru3d_augment_patch_spatial(const float* image, const void* label, int label_dtype, int X, int Y, int Z,
                                          int C, const ru3d_patch_params* p, const ru3d_spatial_params* sp,
                                          const float* lattice, const uint32_t* presence_mask, float* out_image,
                                          int64_t* out_label, void* ws, size_t ws_bytes, void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    RU3D_REQUIRE(p && ws && X > 0 && Y > 0 && Z > 0 && C > 0, "augment_patch_spatial: bad argument");
    RU3D_REQUIRE(sp, "augment_patch_spatial: null spatial params");
    RU3D_REQUIRE((image == nullptr) == (out_image == nullptr), "augment_patch_spatial: image and out_image go together");
    RU3D_REQUIRE((label == nullptr) == (out_label == nullptr), "augment_patch_spatial: label and out_label go together");
    RU3D_REQUIRE(image || label, "augment_patch_spatial: nothing to resample");
    RU3D_REQUIRE(!label || label_dtype == RU3D_LABEL_U8 || label_dtype == RU3D_LABEL_I64,
                 "augment_patch_spatial: bad label dtype %d", label_dtype);
    for (int d = 0; d < 3; d++) RU3D_REQUIRE(p->patch[d] > 0, "augment_patch_spatial: empty patch on axis %d", d);
    RU3D_REQUIRE(ws_bytes >= ru3d_augment_workspace_bytes(p->patch[0], p->patch[1], p->patch[2]),
                 "augment_patch_spatial: workspace too small");
    RU3D_REQUIRE((int64_t)X * Y * Z * C < (1ll << 40), "augment_patch_spatial: volume too large");
    const int64_t total = (int64_t)p->patch[0] * p->patch[1] * p->patch[2];
    RU3D_REQUIRE(total < (1ll << 31), "augment_patch_spatial: patch too large");
    Spatial g;
    for (int d = 0; d < 3; d++) RU3D_REQUIRE(isfinite(sp->centre[d]), "augment_patch_spatial: non-finite centre[%d]", d);
    for (int d = 0; d < 9; d++) RU3D_REQUIRE(isfinite(sp->matrix[d]), "augment_patch_spatial: non-finite matrix[%d]", d);
    g.elastic = sp->lattice[0] || sp->lattice[1] || sp->lattice[2];
    for (int d = 0; d < 3; d++) {
        g.c[d] = sp->centre[d];
        g.patch[d] = p->patch[d];
        g.flip[d] = p->flip[d] != 0;
        g.n[d] = g.elastic ? sp->lattice[d] : 0;
        g.g[d] = g.elastic ? sp->spacing[d] : 1;
        if (!g.elastic) continue;
        RU3D_REQUIRE(sp->spacing[d] >= 4, "augment_patch_spatial: spacing[%d] = %d is below 4", d, sp->spacing[d]);
        const int want = (p->patch[d] - 1 + sp->spacing[d] - 1) / sp->spacing[d] + 3;
        RU3D_REQUIRE(sp->lattice[d] == want, "augment_patch_spatial: lattice[%d] = %d, a patch of %d at spacing %d has %d",
                     d, sp->lattice[d], p->patch[d], sp->spacing[d], want);
    }
    for (int d = 0; d < 9; d++) g.m[d] = sp->matrix[d];
    size_t lds = 12 * sizeof(double);
    if (g.elastic) {
        RU3D_REQUIRE(lattice, "augment_patch_spatial: a lattice is described but the lattice pointer is null");
        RU3D_REQUIRE((int64_t)(g.n[1] + 4) * g.n[2] <= RU3D_SPATIAL_MAX_YZ,
                     "augment_patch_spatial: lattice %d x %d x %d exceeds the LDS budget ((ny + 4) * nz <= %d)", g.n[0],
                     g.n[1], g.n[2], RU3D_SPATIAL_MAX_YZ);
        lds += (size_t)(g.n[1] + 4) * g.n[2] * 3 * sizeof(double);
    }
    g.ychunks = (p->patch[1] + SPATIAL_ROWS - 1) / SPATIAL_ROWS;
    g.groups = p->patch[0] * g.ychunks;
    // one partial per workgroup in the workspace of ru3d_augment_workspace_bytes: rows shorter than 32 voxels share
    // workgroups
    const int64_t slots = (total + 255) / 256;
    const unsigned blocks = (unsigned)(g.groups < slots ? g.groups : slots);
    double* part = (double*)ws;
    if (!label || label_dtype == RU3D_LABEL_U8)
        hipLaunchKernelGGL(spatial_kernel<uint8_t>, dim3(blocks), dim3(256), lds, as_stream(stream), image,
                           (const uint8_t*)label, X, Y, Z, C, g, p->image_cval, p->label_cval, lattice, presence_mask,
                           out_image, out_label, part);
    else
        hipLaunchKernelGGL(spatial_kernel<int64_t>, dim3(blocks), dim3(256), lds, as_stream(stream), image,
                           (const int64_t*)label, X, Y, Z, C, g, p->image_cval, p->label_cval, lattice, presence_mask,
                           out_image, out_label, part);
    int rc = ru3d_check_launch("augment_spatial");
    if (rc) return rc;
    return launch_intensity(image != nullptr, p, out_image, total * C, part, (int)blocks, stream);
}

extern "C" int ru3d_augment_intensity(float* image, int64_t count, const double* part, int nparts,
                                      const ru3d_patch_params* p, void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    RU3D_REQUIRE(image && part && p, "augment_intensity: bad argument");
    RU3D_REQUIRE(count > 0 && nparts > 0, "augment_intensity: empty image or no partials");
    return launch_intensity(true, p, image, count, part, nparts, stream);
}
