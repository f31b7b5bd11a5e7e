"""Exact Euclidean distance transform of a packed mask and the pieces of the surface-distance metrics on the device
(csrc/distance.hip).

What the host pays for a boundary metric is two `scipy.ndimage.distance_transform_edt` of the full volume per class;
here a class is two packed surfaces, two transforms, two gathers and a handful of reductions that never leave HBM.
The transform's contract is a formula, not an algorithm: `out[p] = min_f fl(A + fl(B + C))` with
`A = fl(fl(sx (px - fx))^2)` (B, C alike) in float64, so results can be compared with `==` against a brute force of
the same expression.  Masks are `morphology.PackedMask`.  There is no host fallback in here: every function wants HIP
tensors (the numpy yardstick of the metrics lives in trainer.py).
"""
import ctypes
import math

import numpy as np
import torch

import _native as N
from _native import check, ptr, stream
from morphology import PackedMask

MAX_AXIS = N.EDT_MAX_AXIS
_INITIAL_CAPACITY = 1 << 20             # surface voxels per mask the metric buffers hold before they have to grow
_capacity = {}                          # device -> values per side of the metric buffers


def _packed(mask, what):
    if not isinstance(mask, PackedMask):
        raise ValueError("%s: expected a PackedMask (morphology.pack), got %s" % (what, type(mask).__name__))
    N.require_device(mask.bits, what)
    return mask


def _spacing(sampling, ndim):
    """scipy's `sampling` (None, a number, or one number per axis of the volume) as three floats, leading axes 1."""
    if sampling is None:
        s = (1.0,) * ndim
    elif np.ndim(sampling) == 0:
        s = (float(sampling),) * ndim
    else:
        s = tuple(float(v) for v in sampling)
    if len(s) != ndim:
        raise ValueError("sampling: %d values for a volume of %d axes" % (len(s), ndim))
    if not all(math.isfinite(v) and v > 0 for v in s):
        raise ValueError("sampling: %r (every value finite and > 0)" % (sampling,))
    return (1.0,) * (3 - ndim) + s


def edt_squared(mask, sampling=None):
    """float64 HIP tensor of the mask's shape: the squared distance, in `sampling` units, of every voxel to the nearest
    SET bit of `mask` (the feature voxels); +inf everywhere when no bit is set."""
    if not isinstance(mask, PackedMask):
        raise ValueError("edt_squared: expected a PackedMask (morphology.pack), got %s" % type(mask).__name__)
    X, Y, Z = mask.shape3
    if X > MAX_AXIS or Y > MAX_AXIS:
        raise ValueError("edt_squared: a volume of shape %s is beyond the limit of %d voxels along every axis but the "
                         "last" % (mask.shape, MAX_AXIS))
    spacing = (ctypes.c_double * 3)(*_spacing(sampling, len(mask.shape)))
    N.require_device(mask.bits, "edt_squared")
    out = torch.empty(mask.shape, dtype=torch.float64, device=mask.device)
    nbytes = N.lib.ru3d_edt_workspace_bytes(X, Y, Z)
    ws = N.workspace(nbytes, mask.device)
    N.note_device(mask.device)
    check(N.lib.ru3d_edt_squared(ptr(mask.bits), X, Y, Z, spacing, ptr(out), ptr(ws), ws.numel(), stream()), "edt_squared")
    return out


def surface(mask):
    """`mask & ~erode(mask)` with the 6-neighbour cross and border_value 0 as a new PackedMask: the voxels of the mask
    with a face neighbour outside it (the volume's faces count as outside)."""
    _packed(mask, "surface")
    X, Y, Z = mask.shape3
    out = mask.new()
    N.note_device(mask.device)
    check(N.lib.ru3d_mask_surface(ptr(mask.bits), ptr(out.bits), X, Y, Z, stream()), "mask_surface")
    return out


def _gather_into(sq, query, values, count):
    """Enqueue values[:] = sq[query] (as far as `values` reaches) and count[0] = the number of set bits; no host read."""
    X, Y, Z = query.shape3
    nbytes = N.lib.ru3d_edt_gather_workspace_bytes(X, Y, Z)
    ws = N.workspace(nbytes, query.device)
    N.note_device(query.device)
    check(N.lib.ru3d_edt_gather(ptr(sq), ptr(query.bits), X, Y, Z, ptr(values), 0 if values is None else values.numel(),
                                ptr(count), ptr(ws), ws.numel(), stream()), "edt_gather")


def _check_volume(sq, query, what):
    if not isinstance(query, PackedMask):
        raise ValueError("%s: expected a PackedMask (morphology.pack), got %s" % (what, type(query).__name__))
    if (not torch.is_tensor(sq) or sq.dtype != torch.float64 or tuple(sq.shape) != query.shape
            or sq.device != query.device):
        raise ValueError("%s: sq must be a float64 tensor of shape %s on %s" % (what, query.shape, query.device))
    N.require_device(query.bits, what)
    return sq.contiguous()


def gather(sq, query, capacity=None):
    """numpy's `sq[query]` for a float64 HIP volume and a PackedMask of its shape: the values at the set bits in element
    order, as a float64 HIP vector.  capacity=None reads the number of set bits back first and returns exactly that
    many values; capacity=k enqueues one gather into a buffer of k values without a host read and returns
    (values, count) with count a device int64 [1] - a count above k means the buffer was too small, and nothing was
    written beyond it."""
    sq = _check_volume(sq, query, "gather")
    count = torch.empty(1, dtype=torch.int64, device=query.device)
    if capacity is None:
        _gather_into(None, query, None, count)
        n = int(count.item())
        values = torch.empty(n, dtype=torch.float64, device=query.device)
        if n:
            _gather_into(sq, query, values, count)
        return values
    if int(capacity) < 1:
        raise ValueError("gather: capacity=%r (>= 1)" % (capacity,))
    values = torch.empty(int(capacity), dtype=torch.float64, device=query.device)
    _gather_into(sq, query, values, count)
    return values, count


def reduce(values, count, tolerance_sq):
    """float64 HIP tensor [4]: (n, max, #{v <= tolerance_sq}, sum of sqrt(v)) over the first n = min(count, len(values))
    squared distances; `count` is a device int64 [1] (what `gather(..., capacity=)` returned).  No host read."""
    if (not torch.is_tensor(values) or values.dtype != torch.float64 or values.dim() != 1 or values.numel() < 1
            or not values.is_contiguous()):
        raise ValueError("reduce: values must be a contiguous float64 vector of at least one element")
    N.require_device(values, "reduce: values")
    if not torch.is_tensor(count) or count.dtype != torch.int64 or count.numel() != 1 or count.device != values.device:
        raise ValueError("reduce: count must be an int64 tensor of one element on %s" % values.device)
    if not float(tolerance_sq) >= 0:
        raise ValueError("reduce: tolerance_sq=%r (>= 0)" % (tolerance_sq,))
    out = torch.empty(4, dtype=torch.float64, device=values.device)
    nbytes = N.lib.ru3d_edt_reduce_workspace_bytes(values.numel())
    ws = N.workspace(nbytes, values.device)
    N.note_device(values.device)
    check(N.lib.ru3d_edt_reduce(ptr(values), ptr(count), values.numel(), float(tolerance_sq), ptr(out), ptr(ws), ws.numel(),
                                stream()), "edt_reduce")
    return out


def surface_distances(a, b, sampling=None):
    """Squared distances, in `sampling` units, from every surface voxel of the PackedMask `a` to the nearest surface
    voxel of `b`, in element order of a's surface, as a float64 HIP vector (+inf when b is empty)."""
    _packed(a, "surface_distances")
    _packed(b, "surface_distances")
    if a.shape != b.shape or a.device != b.device:
        raise ValueError("surface_distances: masks of shape %s on %s and %s on %s" % (a.shape, a.device, b.shape, b.device))
    return gather(edt_squared(surface(b), sampling), surface(a))


def surface_stats(a, b, sampling=None, tolerance=1.0, q=95.0):
    """Everything the surface-distance metrics of one class need, from two PackedMasks, with one download of 10 numbers:
    a dict with n_ab, n_ba (surface voxels of a and of b), max_ab, max_ba (largest squared distance from a's surface
    to b's and back), within_ab, within_ba (squared distances <= tolerance * tolerance), sum_ab, sum_ba (sums of the
    distances) and lo, hi (the two order statistics of the concatenated squared distances that the q-th percentile
    interpolates between).  When one surface is empty the distances are not defined and only the counts are filled."""
    _packed(a, "surface_stats")
    _packed(b, "surface_stats")
    if a.shape != b.shape or a.device != b.device:
        raise ValueError("surface_stats: masks of shape %s on %s and %s on %s" % (a.shape, a.device, b.shape, b.device))
    device = a.device
    tol_sq = float(tolerance) * float(tolerance)
    sa, sb = surface(a), surface(b)
    to_b, to_a = edt_squared(sb, sampling), edt_squared(sa, sampling)
    while True:
        cap = _capacity.get(device, _INITIAL_CAPACITY)
        both = torch.full((2 * cap,), float('inf'), dtype=torch.float64, device=device)
        counts = torch.empty(2, dtype=torch.int64, device=device)
        _gather_into(to_b, sa, both[:cap], counts[0:1])
        _gather_into(to_a, sb, both[cap:], counts[1:2])
        red_ab = reduce(both[:cap], counts[0:1], tol_sq)
        red_ba = reduce(both[cap:], counts[1:2], tol_sq)
        # the padding is +inf, so the n = n_ab + n_ba gathered values are the first n of the sorted buffer
        ordered = torch.sort(both).values
        n = counts.clamp(max=cap).sum()
        lo = torch.floor((n - 1).to(torch.float64) * (q / 100.0)).to(torch.int64).clamp(min=0)
        hi = torch.minimum(lo + 1, (n - 1).clamp(min=0))
        picked = ordered[torch.stack((lo, hi))]
        got = torch.cat((counts.to(torch.float64), red_ab[1:], red_ba[1:], picked)).cpu().numpy()     # the one download
        n_ab, n_ba = int(got[0]), int(got[1])
        if max(n_ab, n_ba) <= cap:
            break
        _capacity[device] = 1 << (max(n_ab, n_ba) - 1).bit_length()         # too small: grow and gather once more
    stats = {'n_ab': n_ab, 'n_ba': n_ba}
    if n_ab and n_ba:
        stats.update(max_ab=float(got[2]), within_ab=int(got[3]), sum_ab=float(got[4]), max_ba=float(got[5]),
                     within_ba=int(got[6]), sum_ba=float(got[7]), lo=float(got[8]), hi=float(got[9]))
    return stats
