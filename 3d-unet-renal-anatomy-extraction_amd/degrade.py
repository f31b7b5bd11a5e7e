"""Gaussian noise, Gaussian blur and simulated low resolution: the three image-quality ops of the on-device patch
sampler (kernels: csrc/degrade.hip behind ru3d_augment_degrade; contract: include/ru3d.h).

This module holds what the host side of both routes shares: the argument checks and the host draws of
`augment.DeviceAugment(noise=..., blur=..., low_res=...)`, the numpy twins that define the semantics (re-exported
channels-last by `transform.gaussian_noise / gaussian_blur / simulate_low_resolution`), and the call into the library.
The twins work on channels-first arrays [C, X, Y, Z], the layout of a sampled patch.

Chain order: resample (+ mirror), noise, blur, low-res, contrast, brightness, gamma.  Each op acts on the image only and
on all channels with one parameter set.  Draws, from the sampler's rng, after the mirror draws and before the contrast
draw: for every configured op u = uniform(); the op applies iff u < p, and only then are its parameters drawn - noise:
variance = uniform(lo, hi), k0 = randint(0, 2**31), k1 = randint(0, 2**31); blur: sigma = uniform(lo, hi); low-res:
zoom = uniform(lo, hi).  The usual recipe is noise (0.1, (0, 0.1)), blur (0.2, (0.5, 1.0)), low_res (0.25, (0.5, 1.0));
nothing is on by default.
"""
import ctypes
import math

import numpy as np

MAX_RADIUS = 16                 # RU3D_DEGRADE_MAX_RADIUS


# --------------------------------------------------------------------------------------------------- argument checks
def _check(name, v):
    """None | (p, (lo, hi)) -> None | (p, (lo, hi)) as floats."""
    if v is None:
        return None
    try:
        p, (lo, hi) = v
        p, lo, hi = float(p), float(lo), float(hi)
    except (TypeError, ValueError):
        raise ValueError("%s must be None or (p, (lo, hi)), got %r" % (name, v))
    if not (0.0 <= p <= 1.0):
        raise ValueError("%s: probability %r is outside [0, 1]" % (name, p))
    if not (math.isfinite(lo) and math.isfinite(hi) and lo <= hi):
        raise ValueError("%s: range (%r, %r) is not a finite lo <= hi" % (name, lo, hi))
    return p, (lo, hi)


def blur_radius(sigma):
    """scipy's truncate = 4: taps to either side of the centre."""
    return int(4.0 * float(sigma) + 0.5)


def low_grid(patch, zoom):
    return [max(int(np.round(p * zoom)), 2) for p in patch]


def check_noise(v):
    v = _check("noise", v)
    if v is not None and v[1][0] < 0:
        raise ValueError("noise: the variance range (%r, %r) reaches below 0" % v[1])
    return v


def check_blur(v, patch=None):
    """patch: the extents the blur will run on, when they are known."""
    v = _check("blur", v)
    if v is None:
        return None
    lo, hi = v[1]
    if lo <= 0:
        raise ValueError("blur: sigma range (%r, %r) is not positive" % (lo, hi))
    r = blur_radius(hi)
    if r > MAX_RADIUS:
        raise ValueError("blur: sigma %r gives a radius of %d taps, above the kernel's %d" % (hi, r, MAX_RADIUS))
    if patch is not None and r > min(patch):
        raise ValueError("blur: sigma %r gives a radius of %d taps, above the smallest patch extent %d (one reflection "
                         "at the border would not suffice)" % (hi, r, min(patch)))
    return v


def check_low_res(v, patch=None):
    v = _check("low_res", v)
    if v is None:
        return None
    lo, hi = v[1]
    if not (0 < lo and hi <= 1):
        raise ValueError("low_res: zoom range (%r, %r) is outside (0, 1]" % (lo, hi))
    if patch is not None and min(patch) < 2:
        raise ValueError("low_res: a patch extent of %d has no coarser grid" % min(patch))
    return v


def draw(rng, noise, blur, low_res):
    """The host draws of one patch, in chain order -> {'noise': (variance, (k0, k1)), 'blur': sigma, 'low_res': zoom}
    with the ops that apply."""
    ops = {}
    if noise is not None and rng.uniform() < noise[0]:
        variance = float(rng.uniform(noise[1][0], noise[1][1]))
        k0 = int(rng.randint(0, 2 ** 31))
        ops["noise"] = (variance, (k0, int(rng.randint(0, 2 ** 31))))
    if blur is not None and rng.uniform() < blur[0]:
        ops["blur"] = float(rng.uniform(blur[1][0], blur[1][1]))
    if low_res is not None and rng.uniform() < low_res[0]:
        ops["low_res"] = float(rng.uniform(low_res[1][0], low_res[1][1]))
    return ops


# ------------------------------------------------------------------------------------------------------ numpy twins
_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_LOW = np.uint64(0xFFFFFFFF)
_SHIFT = np.uint64(32)


def philox4x32(counter, key):
    """Philox4x32-10 in numpy integer arithmetic (numpy's own Philox is the 4x64 variant): counter [..., 4] and key (k0, k1)
    of 32-bit words -> uint32 [..., 4]."""
    c = np.asarray(counter, dtype=np.uint64) & _LOW
    c0, c1, c2, c3 = (c[..., k] for k in range(4))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = c0 * np.uint64(_M0), c2 * np.uint64(_M1)             # 32 x 32 bits: no overflow in 64
        c0, c1, c2, c3 = (p1 >> _SHIFT) ^ c1 ^ np.uint64(k0), p1 & _LOW, (p0 >> _SHIFT) ^ c3 ^ np.uint64(k1), p0 & _LOW
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def philox_normals(count, key):
    """float64 standard normals 0 .. count - 1: normal i is number i & 3 of the call with counter (i >> 2, 0, 0, 0)."""
    calls = (int(count) + 3) // 4
    counter = np.zeros((calls, 4), dtype=np.uint64)
    j = np.arange(calls, dtype=np.uint64)
    counter[:, 0], counter[:, 1] = j & _LOW, j >> _SHIFT
    x = philox4x32(counter, key).astype(np.float64)
    out = np.empty((calls, 4), dtype=np.float64)
    for a in (0, 2):
        ua, ub = (x[:, a] + 0.5) * 2.0 ** -32, (x[:, a + 1] + 0.5) * 2.0 ** -32
        radius = np.sqrt(-2.0 * np.log(ua))
        out[:, a], out[:, a + 1] = radius * np.cos(2.0 * np.pi * ub), radius * np.sin(2.0 * np.pi * ub)
    return out.reshape(-1)[:int(count)]


def gaussian_noise(image, variance, key):
    """image float32 [C, X, Y, Z] (any shape: the index runs over the array in C order)."""
    if not (math.isfinite(variance) and variance >= 0):
        raise ValueError("noise: variance %r is not a finite non-negative number" % (variance,))
    x = np.ascontiguousarray(image, dtype=np.float32)
    n = philox_normals(x.size, key).reshape(x.shape)
    return (x.astype(np.float64) + np.sqrt(np.float64(variance)) * n).astype(np.float32)


def blur_weights(sigma):
    """weights at distance 0 .. r, normalised over the whole kernel in float64 (scipy's _gaussian_kernel1d)."""
    r = blur_radius(sigma)
    t = np.arange(-r, r + 1, dtype=np.float64)
    w = np.exp(-0.5 / (float(sigma) * float(sigma)) * t ** 2)
    w /= w.sum()
    return w[r:]


def _blur_axis(a, w, axis):
    r = len(w) - 1
    pad = [(0, 0)] * a.ndim
    pad[axis] = (r, r)
    p = np.moveaxis(np.pad(a, pad, mode="symmetric").astype(np.float64), axis, 0)       # ... b a | a b ...
    n = a.shape[axis]
    acc = p[r:r + n] * w[0]
    for d in range(r, 0, -1):                                                            # scipy's order of taps
        acc = acc + (p[r - d:r - d + n] + p[r + d:r + d + n]) * w[d]
    return np.moveaxis(acc, 0, axis).astype(np.float32)


def gaussian_blur(image, sigma):
    """image float32 [C, X, Y, Z]: every channel through scipy.ndimage.gaussian_filter(sigma) restated - passes along x, y,
    z, each accumulated in float64 and stored as float32.  (No bound on the radius here: numpy reflects as often as it
    takes; the kernels refuse a radius above MAX_RADIUS or above the smallest extent.)"""
    x = np.ascontiguousarray(image, dtype=np.float32)
    if not (math.isfinite(sigma) and sigma > 0):
        raise ValueError("blur: sigma %r is not positive" % (sigma,))
    w = blur_weights(sigma)
    for axis in (-3, -2, -1):
        x = _blur_axis(x, w, axis)
    return x


def low_res_taps(P, n):
    """Per output voxel of an axis of P voxels seen through a low grid of n: (source voxel of low-grid neighbour
    floor(t), of floor(t) + 1, weight t - floor(t)), t = o * ((n - 1) / (P - 1))."""
    up, down = np.float64(n - 1) / np.float64(P - 1), np.float64(P - 1) / np.float64(n - 1)
    t = np.arange(P, dtype=np.float64) * up
    f = np.floor(t)
    l0 = np.clip(f.astype(np.int64), 0, n - 1)
    l1 = np.minimum(l0 + 1, n - 1)
    src = [np.clip(np.floor(l.astype(np.float64) * down + 0.5).astype(np.int64), 0, P - 1) for l in (l0, l1)]
    return src[0], src[1], t - f


def simulate_low_resolution(image, zoom):
    """image float32 [C, X, Y, Z]: every channel nearest-neighbour down to low_grid(patch, zoom) and order 1 back up, what
    transform.resize(resize(x, n, order=0), P, order=1) computes, as one gather in float64 rounded once."""
    x = np.ascontiguousarray(image, dtype=np.float32)
    if not (0 < zoom <= 1):
        raise ValueError("low_res: zoom %r is outside (0, 1]" % (zoom,))
    P = x.shape[-3:]
    if min(P) < 2:
        raise ValueError("low_res: a patch extent of %d has no coarser grid" % min(P))
    taps = [low_res_taps(p, n) for p, n in zip(P, low_grid(P, zoom))]
    shapes = [(-1, 1, 1), (1, -1, 1), (1, 1, -1)]
    out = np.zeros(x.shape, dtype=np.float64)
    for a in (0, 1):
        for b in (0, 1):
            for c in (0, 1):                                  # scipy's order: the last axis fastest
                coeff = x[..., taps[0][a][:, None, None], taps[1][b][None, :, None], taps[2][c][None, None, :]]
                coeff = coeff.astype(np.float64)
                for d, k in enumerate((a, b, c)):
                    wd = taps[d][2] if k else 1.0 - taps[d][2]
                    coeff = coeff * wd.reshape(shapes[d])
                out = out + coeff
    return out.astype(np.float32)


def apply_numpy(image, ops):
    """The ops `draw` returned, in chain order, on a channels-first float32 patch."""
    if "noise" in ops:
        image = gaussian_noise(image, *ops["noise"])
    if "blur" in ops:
        image = gaussian_blur(image, ops["blur"])
    if "low_res" in ops:
        image = simulate_low_resolution(image, ops["low_res"])
    return image


# ----------------------------------------------------------------------------------------------------- device route
def params(ops):
    """-> _native.DegradeParams of the ops `draw` returned."""
    import _native as N
    dg = N.DegradeParams()
    if "noise" in ops:
        dg.do_noise, dg.noise_variance = 1, ops["noise"][0]
        dg.noise_key[:] = [int(k) & 0xFFFFFFFF for k in ops["noise"][1]]
    if "blur" in ops:
        dg.do_blur, dg.blur_sigma = 1, ops["blur"]
    if "low_res" in ops:
        dg.do_low_res, dg.low_res_zoom = 1, ops["low_res"]
    return dg


def workspace(c, patch, device):
    """(partials pointer region, degrade workspace) carved from the stream's scratch buffer: the {sum, min, max} partials
    first (ru3d_augment_workspace_bytes, where the resampling kernels leave theirs), the degrade workspace behind them."""
    import _native as N
    head = (int(N.lib.ru3d_augment_workspace_bytes(*patch)) + 255) // 256 * 256
    tail = int(N.lib.ru3d_augment_degrade_workspace_bytes(c, *patch))
    ws = N.workspace(head + tail, device)
    return ws, ws[head:head + tail]


def launch(image, dg, ws, tail):
    """ru3d_augment_degrade on a contiguous fp32 HIP tensor [C, px, py, pz], in place; the partials land at the start of
    `ws`."""
    import _native as N
    c, px, py, pz = (int(v) for v in image.shape)
    N.note_device(image.device)
    N.check(N.lib.ru3d_augment_degrade(N.ptr(image), c, px, py, pz, ctypes.byref(dg), N.ptr(tail), tail.numel(),
                                       N.ptr(ws), N.stream()), "augment_degrade")


def apply_device(image, ops):
    """The ops on a channels-last fp32 HIP tensor [X, Y, Z, C] (or [X, Y, Z]) -> a new tensor of the same layout."""
    import torch
    import _native as N
    N.require_device(image, "image")
    x = image[..., None] if image.dim() == 3 else image
    if x.dim() != 4:
        raise ValueError("expected an image [X, Y, Z, C] or [X, Y, Z], got shape %s" % (tuple(image.shape),))
    x = x.to(torch.float32).permute(3, 0, 1, 2).contiguous()
    if x.data_ptr() == image.data_ptr():
        x = x.clone()
    ws, tail = workspace(x.shape[0], [int(v) for v in x.shape[1:]], x.device)
    launch(x, params(ops), ws, tail)
    out = x.permute(1, 2, 3, 0).contiguous()
    return out[..., 0] if image.dim() == 3 else out
