"""Morphometry of a label volume (csrc/morphometry.hip): how large every structure is, where it lies, how it is
oriented, its longest diameter, and how much of its surface touches which class.

`ids` is a class volume (uint8) or a component-label volume (int32, `components.label`) of one to three axes; ids
1 .. count are measured, 0 and every value above `count` is skipped.  `moments`, `faces`, `extents`, `candidates` and
`feret` return raw tables: numpy operands take the numpy route, HIP operands the device route, and the device tables
stay on the device.  The tables are integer counts or max / min of float64 values, so the two routes agree exactly
(moments, faces, candidates) or to the rounding of one short float64 sum (extents, feret).  `describe` downloads only
those small tables and turns them, in float64 on the host, into one dict per id.
"""
import ctypes
import math

import numpy as np
import torch

import _native as N
from _native import check, ptr, stream

MAX_VOXELS = 2 ** 31
MAX_OTHER = 256
COLUMNS = ('n', 'x', 'y', 'z', 'xx', 'yy', 'zz', 'xy', 'xz', 'yz')      # of the moments table
_PAIR_CHUNK = 1 << 22           # elements of a block of the numpy route's pair matrix


# ------------------------------------------------------------------------------------------------ operands
def _is_hip(v):
    return torch.is_tensor(v) and v.is_cuda


def _check_shape(shape, what):
    """(X, Y, Z) of a volume of one to three axes; refuses what the kernels refuse, before anything is launched."""
    if len(shape) < 1 or len(shape) > 3:
        raise ValueError("%s: expected a volume of 1 to 3 axes, got shape %s" % (what, tuple(shape)))
    X, Y, Z = (1,) * (3 - len(shape)) + tuple(int(s) for s in shape)
    if min(X, Y, Z) < 1 or X * Y * Z >= MAX_VOXELS:
        raise ValueError("%s: a volume of shape %s is not supported (every extent positive, fewer than 2^31 voxels)"
                         % (what, tuple(shape)))
    if X * Y * Z * (max(X, Y, Z) - 1) ** 2 >= 2 ** 63:
        raise ValueError("%s: the second moments of a volume of shape %s can pass 2^63" % (what, tuple(shape)))
    return X, Y, Z


def _operand(ids, count, what):
    """(volume [X, Y, Z], bytes per id on the device route or None on the numpy route)."""
    count = int(count)
    if count < 0 or count >= MAX_VOXELS:
        raise ValueError("%s: count %d" % (what, count))
    if _is_hip(ids):
        shape = _check_shape(ids.shape, what)
        if ids.dtype == torch.bool:
            ids = ids.contiguous().view(torch.uint8)
        elif ids.dtype not in (torch.uint8, torch.int32):
            if ids.is_floating_point():
                raise ValueError("%s: ids of dtype %s (an integer volume)" % (what, ids.dtype))
            ids = ids.to(torch.int32)
        N.require_device(ids, what)
        return ids.contiguous().reshape(shape), ids.element_size()
    v = np.asarray(ids.numpy() if torch.is_tensor(ids) else ids)
    if v.dtype == np.bool_:
        v = v.view(np.uint8)
    if not np.issubdtype(v.dtype, np.integer):
        raise ValueError("%s: ids of dtype %s (an integer volume)" % (what, v.dtype))
    return v.reshape(_check_shape(v.shape, what)), None


def _other_operand(other, num_other, v, idb, count, what):
    """The class volume the faces are counted against: None = class mode, the ids themselves with classes 0 .. count."""
    if other is None:
        if (idb is not None and idb != 1) or (idb is None and v.dtype != np.uint8):
            raise ValueError("%s: class mode (other=None) wants a uint8 class volume" % what)
        other, num_other = v, count + 1
    num_other = int(num_other)
    if num_other < 0 or num_other > MAX_OTHER:
        raise ValueError("%s: num_other=%d (0 .. %d)" % (what, num_other, MAX_OTHER))
    if count * (num_other + 1) * 3 >= MAX_VOXELS:
        raise ValueError("%s: a table of %d x %d x 3 cells" % (what, count, num_other + 1))
    if idb is not None:
        if not _is_hip(other) or other.device != v.device or other.dtype != torch.uint8 or other.numel() != v.numel():
            raise ValueError("%s: other must be a uint8 tensor of the ids' shape on %s" % (what, v.device))
        return other.contiguous().reshape(v.shape), num_other
    o = np.asarray(other.cpu().numpy() if torch.is_tensor(other) else other)
    if o.dtype != np.uint8 or o.size != v.size:
        raise ValueError("%s: other must be a uint8 volume of the ids' shape" % what)
    return o.reshape(v.shape), num_other


def gram(affine=None, spacing=None):
    """(G00, G11, G22, G01, G02, G12) of G = A^T A, A the 3 x 3 voxel-to-world matrix: d^2 = D^T G D for an index
    difference D, also under an oblique affine."""
    g = _matrix(affine, spacing)[0]
    g = g.T @ g
    return (float(g[0, 0]), float(g[1, 1]), float(g[2, 2]), float(g[0, 1]), float(g[0, 2]), float(g[1, 2]))


def _matrix(affine, spacing):
    """(A float64 [3, 3], origin float64 [3]): the affine's, or diag(spacing), or the identity."""
    if affine is not None:
        affine = np.asarray(affine, dtype=np.float64)
        if affine.shape != (4, 4):
            raise ValueError("affine: shape %s (4 x 4)" % (affine.shape,))
        return affine[:3, :3].copy(), affine[:3, 3].copy()
    if spacing is not None:
        s = np.broadcast_to(np.asarray(spacing, dtype=np.float64), (3,))
        return np.diag(s), np.zeros(3)
    return np.eye(3), np.zeros(3)


# ------------------------------------------------------------------------------------------------ numpy route
def _valid(v, count):
    """(linear indices ascending, ids) of the voxels with 1 <= id <= count, both int64."""
    flat = v.reshape(-1)
    lin = np.flatnonzero((flat >= 1) & (flat <= count)) if count else np.zeros(0, dtype=np.int64)
    return lin.astype(np.int64), flat[lin].astype(np.int64)


def _xyz(lin, shape):
    _, Y, Z = shape
    return lin // (Z * Y), (lin // Z) % Y, lin % Z


def _groups(k):
    """(stable order that sorts the keys, start of every group in that order, key of every group)."""
    order = np.argsort(k, kind='stable')
    ks = k[order]
    starts = np.flatnonzero(np.r_[True, ks[1:] != ks[:-1]]) if ks.size else np.zeros(0, dtype=np.int64)
    return order, starts, ks[starts]


def _moments_numpy(v, count):
    table = np.zeros((count, 10), dtype=np.int64)
    lin, k = _valid(v, count)
    if lin.size:
        x, y, z = _xyz(lin, v.shape)
        order, starts, keys = _groups(k)
        for c, col in enumerate((np.ones_like(x), x, y, z, x * x, y * y, z * z, x * y, x * z, y * z)):
            table[keys - 1, c] = np.add.reduceat(col[order], starts)
    return table


def _faces_numpy(v, count, other, M):
    table = np.zeros(count * (M + 1) * 3, dtype=np.int64)
    if count == 0:
        return table.reshape(0, M + 1, 3)
    v = v.astype(np.int64)
    o = other.astype(np.int64)

    def add(k, col, axis):
        table[:] += np.bincount(((k - 1) * (M + 1) + col) * 3 + axis, minlength=table.size)

    def measured(a):
        return (a >= 1) & (a <= count)

    for axis in range(3):
        n = v.shape[axis]
        for border in (np.take(v, 0, axis=axis), np.take(v, n - 1, axis=axis)):
            add(border[measured(border)], M, axis)
        if n > 1:
            lo = tuple(slice(None, -1) if a == axis else slice(None) for a in range(3))
            hi = tuple(slice(1, None) if a == axis else slice(None) for a in range(3))
            differ = v[lo] != v[hi]
            m = differ & measured(v[lo]) & (o[hi] < M)
            add(v[lo][m], o[hi][m], axis)
            m = differ & measured(v[hi]) & (o[lo] < M)
            add(v[hi][m], o[lo][m], axis)
    return table.reshape(count, M + 1, 3)


def _extents_numpy(v, count, frames):
    out = np.empty((count, 3, 2), dtype=np.float64)
    out[:, :, 0] = np.inf
    out[:, :, 1] = -np.inf
    lin, k = _valid(v, count)
    if lin.size:
        x, y, z = (c.astype(np.float64)[:, None] for c in _xyz(lin, v.shape))
        f = frames[k - 1]
        t = f[:, :, 0] * x + f[:, :, 1] * y + f[:, :, 2] * z + f[:, :, 3]
        order, starts, keys = _groups(k)
        out[keys - 1, :, 0] = np.minimum.reduceat(t[order], starts, axis=0)
        out[keys - 1, :, 1] = np.maximum.reduceat(t[order], starts, axis=0)
    return out


def _candidates_numpy(v, count):
    lin, k = _valid(v, count)
    counts = np.zeros(count, dtype=np.int64)
    if lin.size == 0:
        return np.zeros(0, dtype=np.int32), counts.copy(), counts
    # inside a (row, id) group the linear indices ascend: its first and its last element are the two candidates
    order, starts, _ = _groups((lin // v.shape[2]) * count + (k - 1))
    ends = np.r_[starts[1:], lin.size] - 1
    picked = order[np.unique(np.r_[starts, ends])]
    cl, ck = lin[picked], k[picked]
    by_id = np.lexsort((cl, ck))
    counts = np.bincount(ck - 1, minlength=count).astype(np.int64)
    return cl[by_id].astype(np.int32), np.cumsum(counts) - counts, counts


def dist2(g, d):
    """D^T G D in the order the kernel sums it; g = gram(...), d = integer differences [..., 3]."""
    x, y, z = (np.asarray(d[..., a], dtype=np.float64) for a in range(3))
    g01, g02, g12 = 2.0 * g[3], 2.0 * g[4], 2.0 * g[5]
    return x * (g[0] * x + g01 * y + g02 * z) + y * (g[1] * y + g12 * z) + z * (g[2] * z)


def _feret_numpy(cand, starts, counts, g, shape):
    count = len(counts)
    d2 = np.full(count, -1.0, dtype=np.float64)
    pairs = np.full((count, 6), -1, dtype=np.int32)
    lone = np.flatnonzero(counts == 1)                  # one candidate: one voxel, 0 and the voxel twice
    if lone.size:
        p = np.stack(_xyz(cand[starts[lone]].astype(np.int64), shape), axis=1)
        d2[lone] = 0.0
        pairs[lone] = np.concatenate((p, p), axis=1)
    for k in np.flatnonzero(counts > 1):
        c = cand[starts[k]:starts[k] + counts[k]].astype(np.int64)
        p = np.stack(_xyz(c, shape), axis=1)
        rows = max(1, _PAIR_CHUNK // len(c))
        for i0 in range(0, len(c), rows):
            d = dist2(g, p[i0:i0 + rows, None, :] - p[None, :, :])
            j = int(np.argmax(d))                       # the first maximum: the smallest pair of linear indices
            if d.flat[j] > d2[k]:
                d2[k] = d.flat[j]
                pairs[k] = np.r_[p[i0 + j // len(c)], p[j % len(c)]]
    return d2, pairs


# ------------------------------------------------------------------------------------------------ the tables
def moments(ids, count):
    """int64 [count, 10]: n, Sx, Sy, Sz, Sxx, Syy, Szz, Sxy, Sxz, Syz over the voxel indices of every id (COLUMNS)."""
    v, idb = _operand(ids, count, "moments")
    count = int(count)
    if idb is None:
        return _moments_numpy(v, count)
    X, Y, Z = v.shape
    table = torch.empty((count, 10), dtype=torch.int64, device=v.device)
    if count:
        N.note_device(v.device)
        check(N.lib.ru3d_label_moments(ptr(v), idb, X, Y, Z, count, ptr(table), stream()), "label_moments")
    return table


def faces(ids, count, other=None, num_other=0):
    """int64 [count, num_other + 1, 3]: the faces of every id's voxels by what lies behind them - a voxel of class c of
    `other` (a uint8 volume over the same grid, classes 0 .. num_other - 1) that does not carry the id itself counts in
    column c, the outside of the volume in column num_other - and by the axis of the face.  Values of `other` at or
    above num_other count nowhere.  other=None is class mode: `ids` is its own class volume and num_other = count + 1."""
    v, idb = _operand(ids, count, "faces")
    count = int(count)
    o, M = _other_operand(other, num_other, v, idb, count, "faces")
    if idb is None:
        return _faces_numpy(v, count, o, M)
    X, Y, Z = v.shape
    table = torch.empty((count, M + 1, 3), dtype=torch.int64, device=v.device)
    if count:
        N.note_device(v.device)
        check(N.lib.ru3d_label_faces(ptr(v), idb, ptr(o), M, X, Y, Z, count, ptr(table), stream()), "label_faces")
    return table


def extents(ids, count, frames):
    """float64 [count, 3, 2]: the minimum and the maximum of t = ax x + ay y + az z + b over every id's voxels, for the
    three rows (ax, ay, az, b) of frames[id - 1] (float64 [count, 3, 4]); (+inf, -inf) for an id without a voxel."""
    v, idb = _operand(ids, count, "extents")
    count = int(count)
    frames = frames if torch.is_tensor(frames) else np.asarray(frames, dtype=np.float64)
    if tuple(frames.shape) != (count, 3, 4):
        raise ValueError("extents: frames of shape %s ([%d, 3, 4])" % (tuple(frames.shape), count))
    if idb is None:
        f = frames.cpu().numpy() if torch.is_tensor(frames) else frames
        return _extents_numpy(v, count, np.asarray(f, dtype=np.float64))
    X, Y, Z = v.shape
    f = frames if torch.is_tensor(frames) else torch.from_numpy(np.ascontiguousarray(frames, dtype=np.float64))
    f = f.to(device=v.device, dtype=torch.float64).contiguous()
    out = torch.empty((count, 3, 2), dtype=torch.float64, device=v.device)
    if count:
        N.note_device(v.device)
        check(N.lib.ru3d_label_extents(ptr(v), idb, X, Y, Z, count, ptr(f), ptr(out), stream()), "label_extents")
    return out


def candidates(ids, count):
    """(candidates int32 [total], starts int64 [count], counts int64 [count]): the linear indices of the first and the
    last voxel of every id in every (x, y) row along Z, grouped by id.  The numpy route sorts a group; the device route
    leaves its order undefined.  The device route reads the counts back once, to size the buffer."""
    v, idb = _operand(ids, count, "candidates")
    count = int(count)
    if idb is None:
        return _candidates_numpy(v, count)
    X, Y, Z = v.shape
    counts = torch.empty(count, dtype=torch.int64, device=v.device)
    if count == 0:
        return torch.empty(0, dtype=torch.int32, device=v.device), counts, counts.clone()
    N.note_device(v.device)
    check(N.lib.ru3d_label_feret_count(ptr(v), idb, X, Y, Z, count, ptr(counts), stream()), "label_feret_count")
    starts = torch.cumsum(counts, 0) - counts
    total = int(counts.sum().item())
    cand = torch.empty(total, dtype=torch.int32, device=v.device)
    filled = torch.empty(count, dtype=torch.int64, device=v.device)
    check(N.lib.ru3d_label_feret_fill(ptr(v), idb, X, Y, Z, count, ptr(starts), ptr(filled), ptr(cand) if total else None,
                                      total, stream()), "label_feret_fill")
    return cand, starts, counts


def feret(ids, count, g=None):
    """(d2 float64 [count], pair int32 [count, 6]): the largest squared centre-to-centre distance inside every id under
    the metric g = gram(affine) (None: voxel units), and (x, y, z) of the two voxels that reach it, the smallest pair
    of linear indices on a tie.  One voxel gives 0 and the voxel twice, no voxel -1 and six times -1."""
    g = tuple(float(t) for t in (g if g is not None else (1.0, 1.0, 1.0, 0.0, 0.0, 0.0)))
    if len(g) != 6 or not all(math.isfinite(t) for t in g):
        raise ValueError("feret: g=%r (six finite numbers, gram(affine))" % (g,))
    v, idb = _operand(ids, count, "feret")
    count = int(count)
    cand, starts, counts = candidates(v, count)
    if idb is None:
        return _feret_numpy(cand, starts, counts, g, v.shape)
    X, Y, Z = v.shape
    total = cand.numel()
    d2 = torch.empty(count, dtype=torch.float64, device=v.device)
    pair = torch.empty((count, 6), dtype=torch.int32, device=v.device)
    if count:
        row_d2 = torch.empty(total, dtype=torch.float64, device=v.device)
        row_partner = torch.empty(total, dtype=torch.int32, device=v.device)
        N.note_device(v.device)
        check(N.lib.ru3d_label_feret(ptr(v), idb, X, Y, Z, count, ptr(cand) if total else None, total, ptr(starts),
                                     ptr(counts), (ctypes.c_double * 6)(*g), ptr(row_d2) if total else None,
                                     ptr(row_partner) if total else None, ptr(d2), ptr(pair), stream()), "label_feret")
    return d2, pair


# ------------------------------------------------------------------------------------------------ the report
def _host(t):
    return t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def _principal_axes(cov):
    """(unit axes as rows, largest variance first, the largest component of every axis positive; standard deviations)."""
    w, vec = np.linalg.eigh(cov)
    w, vec = w[::-1], vec[:, ::-1].T
    for a in vec:
        if a[int(np.argmax(np.abs(a)))] < 0:
            a *= -1.0
    return vec, np.sqrt(np.maximum(w, 0.0))


def describe(ids, count, affine=None, spacing=None, other=None, num_other=0):
    """One dict per id 1 .. count, from the tables above (two passes over the volume for the moments and the faces, one
    for the extents along the axes the moments give, and the Feret search); only the tables cross to the host:
      id, voxels, volume_mm3 (n |det A|), centroid_index, centroid_world,
      covariance (world, A C A^T), axes (unit rows, largest variance first), axis_sd, extents_mm (centre to centre
      along the axes), feret_mm with feret_points (world), surface_mm2 (faces of axis d have the area |a_e x a_f|),
      contact_mm2 (per class of `other` and 'outside'), exposed_fraction (surface against class 0 or the outside).
    An id without a voxel has only id and voxels.  affine: 4 x 4 voxel-to-world (oblique ones included); without one,
    `spacing` or voxel units.  other / num_other as in `faces`."""
    count = int(count)
    A, origin = _matrix(affine, spacing)
    tm = _host(moments(ids, count)).astype(np.int64)
    tf = _host(faces(ids, count, other, num_other)).astype(np.int64)
    frames = np.zeros((count, 3, 4), dtype=np.float64)
    out = []
    for k in range(count):
        n, sx, sy, sz, sxx, syy, szz, sxy, sxz, syz = (int(t) for t in tm[k])
        d = {'id': k + 1, 'voxels': n}
        out.append(d)
        if n == 0:
            continue
        s1 = (sx, sy, sz)
        s2 = ((sxx, sxy, sxz), (sxy, syy, syz), (sxz, syz, szz))
        centre = np.array([s / n for s in s1])
        # n S_ab - S_a S_b in exact integers: no cancellation between two large floats
        cov = np.array([[(n * s2[a][b] - s1[a] * s1[b]) / (n * n) for b in range(3)] for a in range(3)])
        world = A @ cov @ A.T
        axes, sd = _principal_axes(world)
        centre_world = A @ centre + origin
        frames[k, :, :3] = axes @ A
        frames[k, :, 3] = axes @ (origin - centre_world)
        d.update(volume_mm3=n * abs(float(np.linalg.det(A))), centroid_index=centre.tolist(),
                 centroid_world=centre_world.tolist(), covariance=world.tolist(), axes=axes.tolist(), axis_sd=sd.tolist())
    te = _host(extents(ids, count, frames))
    d2, pair = (_host(t) for t in feret(ids, count, gram(affine, spacing)))
    area = np.array([np.linalg.norm(np.cross(A[:, 1], A[:, 2])), np.linalg.norm(np.cross(A[:, 0], A[:, 2])),
                     np.linalg.norm(np.cross(A[:, 0], A[:, 1]))])
    M = tf.shape[1] - 1
    for k, d in enumerate(out):
        if d['voxels'] == 0:
            continue
        contact = tf[k].astype(np.float64) @ area
        surface = float(contact.sum())
        d.update(extents_mm=(te[k, :, 1] - te[k, :, 0]).tolist(), feret_mm=math.sqrt(float(d2[k])),
                 feret_points=[(A @ pair[k, :3] + origin).tolist(), (A @ pair[k, 3:] + origin).tolist()],
                 surface_mm2=surface,
                 contact_mm2=dict([(str(c), float(contact[c])) for c in range(M)] + [('outside', float(contact[M]))]),
                 exposed_fraction=(float(contact[0] if M else 0.0) + float(contact[M])) / surface if surface else math.nan)
    return out


def gap_mm(a, b, sampling=None):
    """The smallest centre-to-centre distance between a voxel of mask `a` and a voxel of mask `b` (non-zero = set), in
    `sampling` units; None when one of them is empty.  HIP masks: the exact distance transform of csrc/distance.hip and
    a minimum on the device; numpy masks: scipy's transform."""
    if _is_hip(a) or _is_hip(b):
        import distance
        import morphology
        if not (_is_hip(a) and _is_hip(b)) or a.device != b.device or a.shape != b.shape:
            raise ValueError("gap_mm: two HIP masks of one shape on one device")
        inside = a != 0
        target = morphology.pack(b if b.dtype == torch.uint8 else (b != 0).view(torch.uint8), 'ne', 0)
        sq = distance.edt_squared(target, sampling)
        least = float(torch.where(inside, sq, torch.full_like(sq, math.inf)).min().item()) if inside.numel() else math.inf
        return math.sqrt(least) if math.isfinite(least) else None
    import scipy.ndimage as ndi
    a, b = np.asarray(a) != 0, np.asarray(b) != 0
    if a.shape != b.shape:
        raise ValueError("gap_mm: masks of shape %s and %s" % (a.shape, b.shape))
    if not a.any() or not b.any():
        return None
    return float(ndi.distance_transform_edt(~b, sampling=sampling)[a].min())
