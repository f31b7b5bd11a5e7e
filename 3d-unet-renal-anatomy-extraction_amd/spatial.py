"""Free-form spatial augmentation (rotation, per-axis zoom, cubic B-spline elastic deformation): the geometry, the random
draws and a vectorised numpy resampler.  Pure numpy: the host half of `augment.DeviceAugment(rotation=...,
elastic_spacing=..., elastic_magnitude=...)` (csrc/augment.hip: spatial_kernel) and the whole of
`transform.RandomSpatialCrop`, its twin for DataLoader workers and the yardstick the kernel is held against.

Geometry (include/ru3d.h, ru3d_augment_patch_spatial; everything float64).  Patch P, output voxel o, mirrored index
o'_d = flip_d ? P_d - 1 - o_d : o_d, centred u = o' - (P - 1) / 2:

    s(o) = c + M . (u + D(o'))      M = R . diag(step), step_d = (before_d - 1) / (P_d - 1), c = lo + (before - 1) / 2
    R    = Rz(az) . Ry(ay) . Rx(ax)

with (lo, before) the crop box RandomRescaleCrop draws; R = I, D = 0 is that transform's own coordinate lo + o' * step.
Rotation acts in voxel units (the cases are already resampled to one spacing).  D is a uniform cubic B-spline over a
lattice of control vectors phi[3, nx, ny, nz], n_d = ceil((P_d - 1) / g_d) + 3, in patch voxels.

Draw order (after the scale uniform and the crop-box randints of RandomRescaleCrop, before the mirror and intensity
uniforms): three angle uniforms `uniform(lo, hi)` in axis order - also for axes whose range is (0, 0), and with
rotation=None -, then with an elastic lattice `m = uniform(lo, hi)` and
`phi = (uniform(-1, 1, size=(3, nx, ny, nz)) * m).astype(float32)`.
"""
import numpy as np

MIN_SPACING = 4
MAX_YZ = 2560          # RU3D_SPATIAL_MAX_YZ: (ny + 4) * nz of the lattice, the kernel's LDS budget


# ------------------------------------------------------------------------------------------------ arguments
def check_rotation(rotation):
    """None | r (each axis uniform in [-r, r] radians) | three (lo, hi) pairs -> None | [(lo, hi)] * 3."""
    if rotation is None:
        return None
    if isinstance(rotation, (int, float, np.integer, np.floating)) and not isinstance(rotation, bool):
        r = float(rotation)
        if not np.isfinite(r) or r < 0:
            raise ValueError("rotation: a single number must be finite and non-negative, got %r" % (rotation,))
        return [(-r, r)] * 3
    try:
        pairs = [(float(lo), float(hi)) for lo, hi in rotation]
    except (TypeError, ValueError):
        raise ValueError("rotation: expected None, a number or three (lo, hi) pairs, got %r" % (rotation,)) from None
    if len(pairs) != 3:
        raise ValueError("rotation: expected three (lo, hi) pairs (one per axis), got %d" % len(pairs))
    for lo, hi in pairs:
        if not (np.isfinite(lo) and np.isfinite(hi) and lo <= hi):
            raise ValueError("rotation: every range needs finite lo <= hi, got (%r, %r)" % (lo, hi))
    return pairs


def lattice_shape(patch, spacing):
    """Control points per axis: ceil((P - 1) / g) + 3."""
    return tuple((int(p) - 1 + int(g) - 1) // int(g) + 3 for p, g in zip(patch, spacing))


def check_elastic(elastic_spacing, elastic_magnitude, patch=None):
    """-> None (both None) | ([gx, gy, gz], (lo, hi)).  With `patch` the lattice is held against the kernel's bound."""
    if elastic_spacing is None and elastic_magnitude is None:
        return None
    if elastic_spacing is None or elastic_magnitude is None:
        raise ValueError("elastic_spacing and elastic_magnitude go together: got %r and %r"
                         % (elastic_spacing, elastic_magnitude))
    g = list(elastic_spacing) if isinstance(elastic_spacing, (list, tuple, np.ndarray)) else [elastic_spacing] * 3
    if len(g) != 3 or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in g):
        raise ValueError("elastic_spacing: expected an int or three ints, got %r" % (elastic_spacing,))
    g = [int(v) for v in g]
    if min(g) < MIN_SPACING:
        raise ValueError("elastic_spacing: the control spacing must be at least %d patch voxels, got %r"
                         % (MIN_SPACING, elastic_spacing))
    try:
        lo, hi = (float(v) for v in elastic_magnitude)
    except (TypeError, ValueError):
        raise ValueError("elastic_magnitude: expected (lo, hi) in voxels, got %r" % (elastic_magnitude,)) from None
    if not (np.isfinite(lo) and np.isfinite(hi) and 0 <= lo <= hi):
        raise ValueError("elastic_magnitude: needs 0 <= lo <= hi, got %r" % (elastic_magnitude,))
    if patch is not None:
        n = lattice_shape(patch, g)
        if (n[1] + 4) * n[2] > MAX_YZ:
            raise ValueError("elastic_spacing: %r on a patch of %r makes a lattice of %r control points; the kernel "
                             "takes (ny + 4) * nz <= %d - use a coarser spacing" % (g, tuple(patch), n, MAX_YZ))
    return g, (lo, hi)


# ------------------------------------------------------------------------------------------------ draws
def draw_spatial(rng, rotation, elastic, patch):
    """The draws of one patch in the contract's order -> (angles [3], phi float32 [3, nx, ny, nz] | None)."""
    ranges = rotation if rotation is not None else [(0.0, 0.0)] * 3
    angles = [float(rng.uniform(lo, hi)) for lo, hi in ranges]
    phi = None
    if elastic is not None:
        g, (lo, hi) = elastic
        m = rng.uniform(lo, hi)
        phi = (rng.uniform(-1, 1, size=(3,) + lattice_shape(patch, g)) * m).astype(np.float32)
    return angles, phi


# ------------------------------------------------------------------------------------------------ geometry
def rotation_matrix(ax, ay, az):
    """Rz(az) . Ry(ay) . Rx(ax), right-handed: Rx(a) = [[1, 0, 0], [0, cos a, -sin a], [0, sin a, cos a]], Ry and Rz alike
    (Ry turns z towards x, Rz turns x towards y)."""
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]], dtype=np.float64)
    ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]], dtype=np.float64)
    rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]], dtype=np.float64)
    return rz @ ry @ rx


def patch_geometry(lo, before, patch, angles=(0.0, 0.0, 0.0)):
    """Crop box (lo, before) of RandomRescaleCrop + angles -> (centre [3], matrix [3, 3])."""
    lo, before, patch = (np.asarray(v, dtype=np.float64) for v in (lo, before, patch))
    step = np.where(patch > 1, (before - 1) / np.maximum(patch - 1, 1), 0.0)
    return lo + (before - 1) / 2, rotation_matrix(*angles) @ np.diag(step)


def _bspline_basis(count, g, n):
    """[count, n]: row o holds B_0..B_3(f) at columns i .. i + 3, t = o / g, i = floor(t), f = t - i.  Where (P - 1) / g
    is whole the last voxel has i + 3 == n with weight B_3(0) = 0: as in the kernel that tap goes to the last point."""
    t = np.arange(count, dtype=np.float64) / float(g)
    i = np.floor(t).astype(np.int64)
    f = t - i
    w = np.stack([(1 - f) ** 3, 3 * f ** 3 - 6 * f ** 2 + 4, -3 * f ** 3 + 3 * f ** 2 + 3 * f + 1, f ** 3]) / 6.0
    basis = np.zeros((count, n), dtype=np.float64)
    for a in range(4):
        basis[np.arange(count), np.minimum(i + a, n - 1)] += w[a]
    return basis


def bspline_displacement(phi, spacing, patch):
    """D [3, px, py, pz] float64 at the (unmirrored) patch indices: the tensor-product cubic B-spline of `phi`."""
    phi = np.asarray(phi)
    spacing = [int(v) for v in (spacing if isinstance(spacing, (list, tuple, np.ndarray)) else [spacing] * 3)]
    patch = [int(v) for v in patch]
    if tuple(phi.shape) != (3,) + lattice_shape(patch, spacing):
        raise ValueError("phi: shape %r, a patch of %r at spacing %r has %r"
                         % (tuple(phi.shape), tuple(patch), spacing, (3,) + lattice_shape(patch, spacing)))
    d = phi.astype(np.float64)
    for axis in range(3):         # x, then y, then z, as the kernel collapses the lattice
        basis = _bspline_basis(patch[axis], spacing[axis], phi.shape[1 + axis])
        d = np.moveaxis(np.tensordot(basis, d, axes=(1, 1 + axis)), 0, 1 + axis)
    return d


def spatial_coordinates(patch, centre, matrix, phi=None, spacing=None, flip=None):
    """Source coordinates s(o) float64 [3, px, py, pz] for every output voxel (module docstring)."""
    patch = [int(v) for v in patch]
    q = np.stack(np.meshgrid(*[np.arange(p, dtype=np.float64) - (p - 1) / 2 for p in patch], indexing="ij"))
    if phi is not None:
        q += bspline_displacement(phi, spacing, patch)
    s = np.tensordot(np.asarray(matrix, dtype=np.float64), q, axes=(1, 0))
    s += np.asarray(centre, dtype=np.float64).reshape(3, 1, 1, 1)
    for axis, f in enumerate(flip if flip is not None else ()):
        if f:
            s = np.flip(s, 1 + axis)          # out[o] samples what the unmirrored patch samples at o'
    return np.ascontiguousarray(s)


# ------------------------------------------------------------------------------------------------ resampling
def _lerp(v, wx, wy, wz):
    """v [8, ...] (neighbour k = 4 dx + 2 dy + dz): float64 lerps along axis 0, then 1, then 2 -> float32."""
    a = v[:4] * (1.0 - wx) + v[4:] * wx
    b = a[:2] * (1.0 - wy) + a[2:] * wy
    return (b[0] * (1.0 - wz) + b[1] * wz).astype(np.float32)


def resample_at(input, coords, cval=0, is_label=False, num_classes=None, return_margin=False, chunk=1 << 18):
    """Trilinear gather of `input` at `coords` [3, ...] (voxel coordinates; the volume continued by `cval`, scipy's
    mode='grid-constant').  Image [X, Y, Z] or [X, Y, Z, C] -> float32 coords.shape[1:] (+ (C,)).  Label [X, Y, Z] ->
    its dtype, by the rule of transform.rescale: fewer than three classes (`num_classes`, default highest value present
    + 1): interpolate and truncate; otherwise the neighbour class with the largest interpolated one-hot weight, smallest
    class on ties.  return_margin (labels): also the float64 distance of every voxel from a different answer - top
    weight minus runner-up, or (labels 0 / 1) the distance of the interpolated label from where its float32 becomes 1."""
    input = np.asarray(input)
    coords = np.asarray(coords, dtype=np.float64)
    shape = coords.shape[1:]
    ext = input.shape[:3]
    flat = coords.reshape(3, -1)
    total = flat.shape[1]
    channels = input.shape[3] if input.ndim == 4 else None
    if is_label:
        if num_classes is None:
            num_classes = int(input.max()) + 1
        out = np.empty(total, dtype=input.dtype)
        margin = np.empty(total, dtype=np.float64) if return_margin else None
    else:
        out = np.empty((total, channels or 1), dtype=np.float32)
    vol = input.reshape(-1, channels or 1)
    for start in range(0, total, chunk):
        sl = slice(start, min(start + chunk, total))
        i0, w = [], []
        for d in range(3):
            s = np.clip(flat[d, sl], -2.0, ext[d] + 1.0)
            f = np.floor(s)
            i0.append(f.astype(np.int64))
            w.append(s - f)
        idx = np.empty((8, sl.stop - sl.start), dtype=np.int64)
        inside = np.empty(idx.shape, dtype=bool)
        for k in range(8):
            g = [i0[0] + (k >> 2), i0[1] + ((k >> 1) & 1), i0[2] + (k & 1)]
            inside[k] = ((g[0] >= 0) & (g[0] < ext[0]) & (g[1] >= 0) & (g[1] < ext[1]) & (g[2] >= 0) & (g[2] < ext[2]))
            idx[k] = np.where(inside[k], (g[0] * ext[1] + g[1]) * ext[2] + g[2], 0)
        if not is_label:
            for c in range(channels or 1):
                v = np.where(inside, vol[idx, c].astype(np.float64), float(cval))
                out[sl, c] = _lerp(v, *w)
            continue
        lv = np.where(inside, vol[idx, 0].astype(np.int64), int(cval))
        if num_classes < 3:
            v = _lerp(lv.astype(np.float64), *w)
            out[sl] = v.astype(input.dtype)
            if return_margin:
                v64 = _lerp64(lv.astype(np.float64), *w)
                margin[sl] = np.abs(v64 - (1.0 - 2.0 ** -25))      # labels 0 / 1: below this the float32 is not 1.0
            continue
        tw = np.stack([_lerp((lv == lv[k]).astype(np.float64), *w) for k in range(8)])
        best = tw.max(axis=0)
        res = np.where(tw == best, lv, np.iinfo(np.int64).max).min(axis=0)
        out[sl] = res.astype(input.dtype)
        if return_margin:
            tw64 = np.stack([_lerp64((lv == lv[k]).astype(np.float64), *w) for k in range(8)])
            top = np.where(lv == res, tw64, -1.0).max(axis=0)
            margin[sl] = top - np.where(lv != res, tw64, 0.0).max(axis=0)
    if is_label:
        out = out.reshape(shape)
        return (out, margin.reshape(shape)) if return_margin else out
    return out.reshape(shape + (channels,)) if channels else out.reshape(shape)


def _lerp64(v, wx, wy, wz):
    a = v[:4] * (1.0 - wx) + v[4:] * wx
    b = a[:2] * (1.0 - wy) + a[2:] * wy
    return b[0] * (1.0 - wz) + b[1] * wz
