// Pictures of a case that lives in HBM: a table of slice tiles painted into an RGB8 canvas in one launch, and an
// orthographic ray cast of a label volume with front-to-back compositing of shaded surface events.
// The contract (pixel -> voxel map, grey window, integer blend, sample positions, surface events, normal, shade and
// compositing expressions) is written down in include/ru3d.h; the float64 parts are compiled with contraction off and
// spelled in the contract's order, so visualize.py's numpy restatement can be compared with ==.
//
//   rd_tiles_kernel     persistent grid over chunks of 256 tile pixels; the chunk -> tile map is a prefix over the tile
//                       table held in LDS (one walk of at most 256 records per workgroup).  One pixel per lane: one
//                       gather of the base voxel, per overlay one gather plus four for an outline, three byte stores.
//   rd_prepare_kernel   one mask word (64 voxels of z) per lane: drawn(label) looked up in an LDS copy of the table's
//                       alpha column, the word stored in the packed layout of bitvol.h, and a 1 stored into the
//                       byte of every 8 x 8 x 8 brick the word touches (same value from every writer: no atomics).
//   rd_surface_kernel   16 x 16 pixels per workgroup, 8 x 8 per wave so that neighbouring rays share bricks, mask words
//                       and label lines.  Per ray: clip to the volume (slab test with a margin of two samples), then
//                       walk sample numbers n; a sample in an empty brick jumps to a later n (an estimate of the
//                       brick's exit, accepted only after the contract's position of the last sample passed over has
//                       been checked to lie in the same brick), a sample whose mask bit is clear costs one 8-byte read, a drawn
//                       sample one label byte more, an event the 26 labels around it.  Positions are always
//                       recomputed from n with the contract's expression, never accumulated, so every visited sample is
//                       a sample of the contract and the skipped ones cannot hold an event.
// Every store is guarded by the caller's extents and every voxel index is range-checked before it is used.
#include <math.h>
#include "common.h"
#include "bitvol.h"

#pragma clang fp contract(off)

typedef unsigned long long rd_u64;

#define RD_THREADS 256
#define RD_BRICK 8

// ---------------------------------------------------------------------------------------------------- slice tiles
__device__ __forceinline__ bool rd_tile_ok(const ru3d_render_tile& t) {
    if (!t.volume || t.w <= 0 || t.h <= 0 || t.X <= 0 || t.Y <= 0 || t.Z <= 0 || t.C <= 0) return false;
    if ((long long)t.X * t.Y * t.Z * t.C >= (1ll << 31) || (long long)t.w * t.h >= (1ll << 31)) return false;
    if (t.axis < 0 || t.axis > 2) return false;
    const int extent = t.axis == 0 ? t.X : t.axis == 1 ? t.Y : t.Z;
    if (t.index < 0 || t.index >= extent) return false;
    if (t.kind == RU3D_TILE_F32) return t.channel >= 0 && t.channel < t.C && ((uintptr_t)t.volume & 3) == 0;
    return t.kind == RU3D_TILE_U8 && t.C == 1 && t.table;
}

__device__ __forceinline__ int rd_label(const uint8_t* __restrict__ v, int X, int Y, int Z, int i, int j, int k) {
    if ((unsigned)i >= (unsigned)X || (unsigned)j >= (unsigned)Y || (unsigned)k >= (unsigned)Z) return 0;
    return v[((long long)i * Y + j) * Z + k];
}

__global__ __launch_bounds__(RD_THREADS) void rd_tiles_kernel(const ru3d_render_tile* __restrict__ tiles, int num_tiles,
                                                              uint8_t* __restrict__ canvas, int H, int W) {
    __shared__ long long s_first[RU3D_RENDER_MAX_TILES + 1];      // chunks in front of tile i
    if (threadIdx.x == 0) {
        long long acc = 0;
        for (int i = 0; i < num_tiles; i++) {
            s_first[i] = acc;
            if (rd_tile_ok(tiles[i])) acc += ((long long)tiles[i].w * tiles[i].h + RD_THREADS - 1) / RD_THREADS;
        }
        s_first[num_tiles] = acc;
    }
    __syncthreads();
    const long long chunks = s_first[num_tiles];
    for (long long chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
        int lo = 0, hi = num_tiles;                                // the last tile with s_first <= chunk that owns chunks
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (s_first[mid] <= chunk) lo = mid; else hi = mid;
        }
        const ru3d_render_tile t = tiles[lo];
        const long long p = (chunk - s_first[lo]) * RD_THREADS + threadIdx.x;
        if (s_first[lo + 1] == s_first[lo] || p >= (long long)t.w * t.h) continue;
        const int r = (int)(p / t.w), c = (int)(p % t.w);
        const int cy = t.y0 + r, cx = t.x0 + c;
        if (cy < 0 || cy >= H || cx < 0 || cx >= W) continue;
        const double fa = floor(t.origin[0] + (double)r * t.step[0]), fb = floor(t.origin[1] + (double)c * t.step[1]);
        const int ea = t.axis == 0 ? t.Y : t.X, eb = t.axis == 2 ? t.Y : t.Z;
        int rgb[3] = {0, 0, 0};
        if (fa >= 0.0 && fa < (double)ea && fb >= 0.0 && fb < (double)eb) {
            const int a = (int)fa, b = (int)fb;
            // the voxel, and which axis a step along the tile's rows (da) and columns (db) moves
            const int v[3] = {t.axis == 0 ? t.index : a, t.axis == 1 ? t.index : (t.axis == 0 ? a : b),
                              t.axis == 2 ? t.index : b};
            const int da[3] = {t.axis != 0, t.axis == 0, 0}, db[3] = {0, t.axis == 2, t.axis != 2};
            const long long at = ((long long)v[0] * t.Y + v[1]) * t.Z + v[2];
            if (t.kind == RU3D_TILE_F32) {
                const double val = (double)((const float*)t.volume)[at * t.C + t.channel];
                double s = (val - t.vmin) / (t.vmax - t.vmin);
                if (!(s > 0.0)) s = 0.0;
                if (s > 1.0) s = 1.0;
                rgb[0] = rgb[1] = rgb[2] = (int)floor(255.0 * s + 0.5);
            } else {
                const uint8_t* e = t.table + 4 * (int)((const uint8_t*)t.volume)[at];
                rgb[0] = e[0]; rgb[1] = e[1]; rgb[2] = e[2];
            }
#pragma unroll
            for (int o = 0; o < 2; o++) {
                const uint8_t* ov = t.overlay[o];
                if (!ov || !t.overlay_table[o]) continue;
                const int l = ov[at];
                const uint8_t* e = t.overlay_table[o] + 4 * l;
                const int A = e[3];
                if (A == 0) continue;
                if (t.overlay_mode[o] == RU3D_OVERLAY_OUTLINE) {
                    const bool edge = rd_label(ov, t.X, t.Y, t.Z, v[0] - da[0], v[1] - da[1], v[2] - da[2]) != l ||
                                      rd_label(ov, t.X, t.Y, t.Z, v[0] + da[0], v[1] + da[1], v[2] + da[2]) != l ||
                                      rd_label(ov, t.X, t.Y, t.Z, v[0] - db[0], v[1] - db[1], v[2] - db[2]) != l ||
                                      rd_label(ov, t.X, t.Y, t.Z, v[0] + db[0], v[1] + db[1], v[2] + db[2]) != l;
                    if (!edge) continue;
                }
#pragma unroll
                for (int q = 0; q < 3; q++) rgb[q] = (A * (int)e[q] + (255 - A) * rgb[q] + 127) / 255;
            }
        }
        uint8_t* dst = canvas + ((long long)cy * W + cx) * 3;
        dst[0] = (uint8_t)rgb[0]; dst[1] = (uint8_t)rgb[1]; dst[2] = (uint8_t)rgb[2];
    }
}

extern "C" int ru3d_render_tiles(const ru3d_render_tile* tiles, int num_tiles, uint8_t* canvas, int H, int W,
                                 void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    RU3D_REQUIRE(tiles && canvas, "render_tiles: bad argument (null pointer)");
    RU3D_REQUIRE(((uintptr_t)tiles & 7) == 0, "render_tiles: the tile table must be 8-byte aligned");
    RU3D_REQUIRE(num_tiles >= 1 && num_tiles <= RU3D_RENDER_MAX_TILES, "render_tiles: %d tiles (1 .. %d)", num_tiles,
                 RU3D_RENDER_MAX_TILES);
    RU3D_REQUIRE(H >= 1 && W >= 1 && (int64_t)H * W * 3 < ((int64_t)1 << 31),
                 "render_tiles: a %dx%d canvas is not supported (positive, H*W*3 < 2^31)", H, W);
    const int blocks = ru3d_get_cu_budget() * 8;
    hipLaunchKernelGGL(rd_tiles_kernel, dim3(blocks > 0 ? blocks : 8), dim3(RD_THREADS), 0, as_stream(stream), tiles,
                       num_tiles, canvas, H, W);
    return ru3d_check_launch("render_tiles");
}

// ---------------------------------------------------------------------------------------------------- surface views
struct rd_dims {
    int X, Y, Z, W;                       // W words per voxel row
    int BX, BY, BZ;                       // bricks per axis; BZ = 8 W (a word is eight bricks long)
};
static inline rd_dims rd_make_dims(int X, int Y, int Z) {
    rd_dims g;
    g.X = X; g.Y = Y; g.Z = Z;
    g.W = bv_words(Z);
    g.BX = (X + RD_BRICK - 1) / RD_BRICK;
    g.BY = (Y + RD_BRICK - 1) / RD_BRICK;
    g.BZ = g.W * 8;
    return g;
}
static inline size_t rd_mask_bytes(const rd_dims& g) { return bv_align((size_t)g.X * g.Y * g.W * 8); }
static inline size_t rd_brick_bytes(const rd_dims& g) { return bv_align((size_t)g.BX * g.BY * g.BZ); }

__global__ __launch_bounds__(RD_THREADS) void rd_prepare_kernel(const uint8_t* __restrict__ labels, rd_dims g,
                                                                const uint8_t* __restrict__ table,
                                                                rd_u64* __restrict__ mask, uint8_t* __restrict__ bricks) {
    __shared__ uint8_t s_drawn[256];
    s_drawn[threadIdx.x] = threadIdx.x != 0 && table[4 * threadIdx.x + 3] != 0;
    __syncthreads();
    const long long words = (long long)g.X * g.Y * g.W;
    for (long long wi = (long long)blockIdx.x * RD_THREADS + threadIdx.x; wi < words; wi += (long long)gridDim.x * RD_THREADS) {
        const int w = (int)(wi % g.W);
        const long long row = wi / g.W;
        const int y = (int)(row % g.Y), x = (int)(row / g.Y);
        const uint8_t* src = labels + row * g.Z + (long long)w * 64;
        const int count = g.Z - w * 64 < 64 ? g.Z - w * 64 : 64;
        rd_u64 word = 0;
        if (count == 64 && ((uintptr_t)src & 7) == 0) {
#pragma unroll
            for (int q = 0; q < 8; q++) {
                const rd_u64 eight = ((const rd_u64*)src)[q];
#pragma unroll
                for (int b = 0; b < 8; b++) word |= (rd_u64)s_drawn[(eight >> (8 * b)) & 0xff] << (8 * q + b);
            }
        } else {
            for (int b = 0; b < count; b++) word |= (rd_u64)s_drawn[src[b]] << b;
        }
        mask[wi] = word;
        if (word) {
            uint8_t* dst = bricks + ((long long)(x / RD_BRICK) * g.BY + y / RD_BRICK) * g.BZ + w * 8;
#pragma unroll
            for (int q = 0; q < 8; q++)
                if ((word >> (8 * q)) & 0xff) dst[q] = 1;
        }
    }
}

__device__ __forceinline__ double rd_pos(double base, int n, double dw) { return base + (double)n * dw; }

__global__ __launch_bounds__(RD_THREADS) void rd_surface_kernel(const uint8_t* __restrict__ labels, rd_dims g,
                                                                const uint8_t* __restrict__ table, ru3d_render_view vw,
                                                                const rd_u64* __restrict__ mask,
                                                                const uint8_t* __restrict__ bricks,
                                                                uint8_t* __restrict__ rgb, int* __restrict__ depth, int H,
                                                                int W) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int u = blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7), v = blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
    if (u >= W || v >= H) return;
    const int ext[3] = {g.X, g.Y, g.Z};
    double base[3];
#pragma unroll
    for (int c = 0; c < 3; c++) base[c] = (vw.o[c] + (double)u * vw.du[c]) + (double)v * vw.dv[c];
    // the samples that can lie inside the volume: n_lo <= n < n_hi, two samples of margin on either side
    double tmin = 0.0, tmax = (double)vw.num_steps;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        if (vw.dw[c] == 0.0) {
            if (!(base[c] >= 0.0 && base[c] < (double)ext[c])) tmax = -1.0;
        } else {
            const double t0 = (0.0 - base[c]) / vw.dw[c], t1 = ((double)ext[c] - base[c]) / vw.dw[c];
            tmin = fmax(tmin, fmin(t0, t1));
            tmax = fmin(tmax, fmax(t0, t1));
        }
    }
    int n = 0, n_hi = 0;
    if (tmax >= tmin) {
        n = (int)fmax(0.0, floor(tmin) - 2.0);
        n_hi = (int)fmin((double)vw.num_steps, ceil(tmax) + 3.0);
    }
    double T = 1.0, C[3] = {0.0, 0.0, 0.0};
    int first = -1, prev = 0;
    while (n < n_hi) {
        double q[3];
        int p[3];
        bool inside = true;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            q[c] = rd_pos(base[c], n, vw.dw[c]);
            const double f = floor(q[c]);
            inside = inside && f >= 0.0 && f < (double)ext[c];
            p[c] = inside ? (int)f : 0;
        }
        if (!inside) { prev = 0; n++; continue; }
        const int bz = p[2] >> 3;
        if (!bricks[((long long)(p[0] >> 3) * g.BY + (p[1] >> 3)) * g.BZ + bz]) {
            // an estimate of the samples to the exit of this empty brick, in real arithmetic from q.  It is only an
            // estimate: where |dw_c| is below an ulp of the coordinate, the contract's rounded positions cross a brick
            // face at another sample than the real line does.  So the jump is accepted only if the last sample it
            // passes over, n + jump - 1, lies in this brick as the contract places it: every component of
            // fl(base + fl(n * dw)) is monotone in n, hence so do all samples between; otherwise one step.
            double t = 1048576.0;
            const int b[3] = {p[0] >> 3, p[1] >> 3, bz};
#pragma unroll
            for (int c = 0; c < 3; c++) {
                if (vw.dw[c] > 0.0) t = fmin(t, ((double)(b[c] * RD_BRICK + RD_BRICK) - q[c]) / vw.dw[c]);
                else if (vw.dw[c] < 0.0) t = fmin(t, ((double)(b[c] * RD_BRICK) - q[c]) / vw.dw[c]);
            }
            int jump = (int)floor(t) - 1;
            if (jump > 1) {
                bool same = true;
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    const double e = rd_pos(base[c], n + jump - 1, vw.dw[c]);
                    same = same && e >= (double)(b[c] * RD_BRICK) && e < (double)(b[c] * RD_BRICK + RD_BRICK);
                }
                if (!same) jump = 1;
            }
            prev = 0;
            n += jump > 1 ? jump : 1;
            continue;
        }
        const long long row = (long long)p[0] * g.Y + p[1];
        if (!((mask[row * g.W + (p[2] >> 6)] >> (p[2] & 63)) & 1ull)) { prev = 0; n++; continue; }
        const int L = labels[row * g.Z + p[2]];
        if (L != prev) {
            int gr[3] = {0, 0, 0};
            for (int dx = -1; dx <= 1; dx++)
                for (int dy = -1; dy <= 1; dy++)
#pragma unroll
                    for (int dz = -1; dz <= 1; dz++) {
                        const int occ = rd_label(labels, g.X, g.Y, g.Z, p[0] + dx, p[1] + dy, p[2] + dz) == L;
                        gr[0] += dx * occ; gr[1] += dy * occ; gr[2] += dz * occ;
                    }
            double m[3];
#pragma unroll
            for (int c = 0; c < 3; c++) m[c] = (double)(-gr[c]) / vw.spacing[c];
            const double dot = (m[0] * vw.light[0] + m[1] * vw.light[1]) + m[2] * vw.light[2];
            const double len2 = (m[0] * m[0] + m[1] * m[1]) + m[2] * m[2];
            const double shade = len2 == 0.0 ? vw.ambient + vw.diffuse
                                             : vw.ambient + (vw.diffuse * fmax(dot, 0.0)) / sqrt(len2);
            const uint8_t* e = table + 4 * L;
            const double a = (double)e[3] / 255.0;
            const double k = (T * a) * shade;
#pragma unroll
            for (int c = 0; c < 3; c++) C[c] = C[c] + k * (double)e[c];
            T = T * (1.0 - a);
            if (first < 0) first = n;
            if (T < 0.00390625) break;
        }
        prev = L;
        n++;
    }
    uint8_t* dst = rgb + ((long long)v * W + u) * 3;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const double x = C[c] + T * vw.background[c];
        dst[c] = (uint8_t)(int)floor(fmin(fmax(x, 0.0), 255.0) + 0.5);
    }
    depth[(long long)v * W + u] = first;
}

extern "C" size_t ru3d_render_surface_workspace_bytes(int X, int Y, int Z) {
    if (!bv_shape_ok(X, Y, Z)) return 0;
    const rd_dims g = rd_make_dims(X, Y, Z);
    return rd_mask_bytes(g) + rd_brick_bytes(g);
}

extern "C" int ru3d_render_surface_prepare(const uint8_t* labels, int X, int Y, int Z, const uint8_t* table, void* ws,
                                           size_t ws_bytes, void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    BV_REQUIRE_SHAPE("render_surface_prepare");
    RU3D_REQUIRE(labels && table && ws, "render_surface_prepare: bad argument (null pointer)");
    RU3D_REQUIRE(((uintptr_t)ws & 7) == 0, "render_surface_prepare: the workspace must be 8-byte aligned");
    const rd_dims g = rd_make_dims(X, Y, Z);
    const size_t need = rd_mask_bytes(g) + rd_brick_bytes(g);
    RU3D_REQUIRE(ws_bytes >= need, "render_surface_prepare: workspace of %zu bytes, %zu needed", ws_bytes, need);
    hipStream_t st = as_stream(stream);
    uint8_t* bricks = (uint8_t*)ws + rd_mask_bytes(g);
    if (hipMemsetAsync(bricks, 0, rd_brick_bytes(g), st) != hipSuccess) return ru3d_check_launch("render_surface_prepare");
    const int64_t words = (int64_t)g.X * g.Y * g.W, cap = (int64_t)ru3d_get_cu_budget() * 8;
    int64_t blocks = (words + RD_THREADS - 1) / RD_THREADS;
    blocks = blocks > cap && cap > 0 ? cap : blocks;
    hipLaunchKernelGGL(rd_prepare_kernel, dim3((unsigned)blocks), dim3(RD_THREADS), 0, st, labels, g, table, (rd_u64*)ws,
                       bricks);
    return ru3d_check_launch("render_surface_prepare");
}

extern "C" int ru3d_render_surface(const uint8_t* labels, int X, int Y, int Z, const uint8_t* table,
                                   const ru3d_render_view* view, uint8_t* rgb, int32_t* depth, int H, int W, const void* ws,
                                   size_t ws_bytes, void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    BV_REQUIRE_SHAPE("render_surface");
    RU3D_REQUIRE(labels && table && view && rgb && depth && ws, "render_surface: bad argument (null pointer)");
    RU3D_REQUIRE(((uintptr_t)ws & 7) == 0 && ((uintptr_t)depth & 3) == 0,
                 "render_surface: the workspace must be 8-byte aligned and the depth image 4-byte aligned");
    RU3D_REQUIRE(H >= 1 && W >= 1 && (int64_t)H * W * 3 < ((int64_t)1 << 31),
                 "render_surface: a %dx%d picture is not supported (positive, H*W*3 < 2^31)", H, W);
    RU3D_REQUIRE(view->num_steps >= 0 && view->num_steps <= (1 << 20), "render_surface: %d steps (0 .. 2^20)",
                 view->num_steps);
    bool finite = isfinite(view->ambient) && isfinite(view->diffuse);
    for (int c = 0; c < 3; c++)
        finite = finite && isfinite(view->o[c]) && isfinite(view->du[c]) && isfinite(view->dv[c]) && isfinite(view->dw[c]) &&
                 isfinite(view->light[c]) && isfinite(view->background[c]) && isfinite(view->spacing[c]) &&
                 view->spacing[c] > 0.0;
    RU3D_REQUIRE(finite, "render_surface: the view holds a value that is not finite, or a spacing that is not positive");
    const rd_dims g = rd_make_dims(X, Y, Z);
    const size_t need = rd_mask_bytes(g) + rd_brick_bytes(g);
    RU3D_REQUIRE(ws_bytes >= need, "render_surface: workspace of %zu bytes, %zu needed", ws_bytes, need);
    hipLaunchKernelGGL(rd_surface_kernel, dim3((W + 15) / 16, (H + 15) / 16), dim3(RD_THREADS), 0, as_stream(stream), labels,
                       g, table, *view, (const rd_u64*)ws, (const uint8_t*)ws + rd_mask_bytes(g), rgb, depth, H, W);
    return ru3d_check_launch("render_surface");
}
