"""Local thickness of a packed mask on the device (csrc/thickness.hip): for every voxel of a structure the diameter of
the largest ball that fits inside the structure and contains the voxel (Hildebrand and Rueegsegger 1997) - the calibre
of a vessel at every lumen voxel, the thickness of the parenchyma, of a cyst's wall, of the thinnest bridge.

The contract is a formula (include/ru3d.h, "local thickness"): R2(p) is `distance.edt_squared` of the complement, and
`T2(x) = max { R2(p) : p in M, d2(x, p) < R2(p) }` with d2 the float64 expression of the distance transform, so results
compare with `==` against the brute force of the same expression (transform._local_thickness_numpy), and a maximum
does not depend on the order of its operands: the same bytes in every run.  Distances run between voxel centres, so a
slab of k voxels reads k voxels thick for even k and k + 1 for odd k; this is not corrected for.  Masks are
`morphology.PackedMask`.  There is no host fallback in here: every function wants HIP tensors (the numpy route lives in
transform.py and trainer.py).
"""
import ctypes

import torch

import _native as N
from _native import check, ptr, stream
from distance import MAX_AXIS, _check_volume, _gather_into, _packed, _spacing, edt_squared
from morphology import PackedMask
from skeleton import complement

# (voxels tested against the contract's expression, atomic updates issued) of the last local_squared(count_work=True) of
# this process; None after a call that did not ask for them
last_work = None


def _limits(mask, what):
    if not isinstance(mask, PackedMask):
        raise ValueError("%s: expected a PackedMask (morphology.pack), got %s" % (what, type(mask).__name__))
    X, Y, _ = mask.shape3
    if X > MAX_AXIS or Y > MAX_AXIS:
        raise ValueError("%s: a volume of shape %s is beyond the limit of %d voxels along every axis but the last"
                         % (what, mask.shape, MAX_AXIS))
    N.require_device(mask.bits, what)


def inscribed_squared(mask, sampling=None):
    """float64 HIP tensor of the mask's shape: R2, the squared distance in `sampling` units of every voxel to the nearest
    CLEAR voxel of `mask` inside the volume (0 on the clear voxels themselves; +inf everywhere when every bit is set).
    It is distance.edt_squared of the complement, whose padding bits at z >= Z are clear."""
    _limits(mask, "inscribed_squared")
    return edt_squared(complement(mask), sampling)


def candidates(mask):
    """int32 HIP vector: the linear indices (x Y + y) Z + z of the mask's voxels in element order.  One host read (the
    count)."""
    _packed(mask, "candidates")
    X, Y, Z = mask.shape3
    count = torch.empty(1, dtype=torch.int64, device=mask.device)
    index = torch.empty(X * Y * Z, dtype=torch.int32, device=mask.device)
    ws = N.workspace(N.lib.ru3d_thickness_workspace_bytes(X, Y, Z), mask.device)
    N.note_device(mask.device)
    check(N.lib.ru3d_thickness_candidates(ptr(mask.bits), X, Y, Z, ptr(index), index.numel(), ptr(count), ptr(ws),
                                          ws.numel(), stream()), "thickness_candidates")
    return index[:int(count.item())]


def sort_candidates(r2, index):
    """`index` in the order of descending r2[index] (stable: equal radii keep their element order), on the device."""
    if index.numel() < 2:
        return index
    order = torch.sort(r2.reshape(-1)[index.to(torch.int64)], descending=True, stable=True).indices
    return index[order].contiguous()


def paint(r2, index, shape, sampling=None, count_work=False):
    """T2 (float64 HIP tensor of `shape`) from the float64 volume r2 and the int32 list of candidates, in the order of
    the list; with count_work also the int64 HIP vector [2] of the two work counters, else None."""
    X, Y, Z = (1,) * (3 - len(shape)) + tuple(shape)
    spacing = (ctypes.c_double * 3)(*_spacing(sampling, len(shape)))
    out = torch.empty(tuple(shape), dtype=torch.float64, device=r2.device)
    work = torch.empty(2, dtype=torch.int64, device=r2.device) if count_work else None
    N.note_device(r2.device)
    check(N.lib.ru3d_thickness_paint(ptr(r2), ptr(index), index.numel(), X, Y, Z, spacing, ptr(out), ptr(work), stream()),
          "thickness_paint")
    return out, work


def local_squared(mask, sampling=None, presort=True, count_work=False):
    """float64 HIP tensor of the mask's shape: T2, the squared radius in `sampling` units of the largest inscribed ball
    that contains the voxel; 0 outside the mask, +inf everywhere when every bit is set.  presort paints the large balls
    first (one device sort of the candidates by descending R2), so that most later tests end at a plain load;
    presort=False paints in element order: the same bytes, more atomics.  count_work=True leaves the two work counters
    of the paint in `last_work` (one more host read)."""
    global last_work
    _limits(mask, "local_squared")
    _spacing(sampling, len(mask.shape))
    r2 = inscribed_squared(mask, sampling)
    index = candidates(mask)
    if presort:
        index = sort_candidates(r2, index)
    out, work = paint(r2, index, mask.shape, sampling, count_work)
    last_work = tuple(int(v) for v in work.tolist()) if count_work else None
    return out


def diameter(t2):
    """2 sqrt(T2): the local thickness in the unit of the sampling, from the tensor of local_squared."""
    if not torch.is_tensor(t2) or t2.dtype != torch.float64:
        raise ValueError("diameter: t2 must be the float64 tensor of local_squared")
    return 2.0 * torch.sqrt(t2)


def summary(t2, mask, q=(5, 50, 95)):
    """Statistics of T2 over the voxels of `mask`, with one download: a dict with n (the voxels), t2_min and t2_max, order
    (per percentile of q the two order statistics (lo, hi) of T2 that np.percentile interpolates between, by the rank
    rule of trainer._percentile_ranks - the host takes their square roots and interpolates), and mean and std (the
    population standard deviation) of the thickness 2 sqrt(T2).  An empty mask gives n = 0 alone.  Where T2 is +inf (a mask
    that fills its volume) the mean is inf and std is nan.  The buffer that is sorted has the volume's size, whatever the
    structure's."""
    t2 = _check_volume(t2, mask, "summary")
    q = tuple(float(v) for v in q)
    if not all(0.0 <= v <= 100.0 for v in q):
        raise ValueError("summary: q=%r (percentiles 0 .. 100)" % (q,))
    device = mask.device
    cap = t2.numel()
    values = torch.full((cap,), float('inf'), dtype=torch.float64, device=device)
    count = torch.empty(1, dtype=torch.int64, device=device)
    _gather_into(t2, mask, values, count)
    # the padding is +inf, so the n gathered values are the first n of the sorted buffer
    ordered = torch.sort(values).values
    n = count[0]
    last = (n - 1).clamp(min=0)
    ranks = [last, last * 0]
    for v in q:
        lo = torch.floor((n - 1).to(torch.float64) * (v / 100.0)).to(torch.int64).clamp(min=0)
        ranks += [lo, torch.minimum(lo + 1, last)]
    picked = ordered[torch.stack(ranks)]
    inside = torch.arange(cap, device=device) < n
    thick = torch.where(inside, 2.0 * torch.sqrt(ordered), torch.zeros_like(ordered))
    nf = n.clamp(min=1).to(torch.float64)
    mean = thick.sum() / nf
    var = (torch.where(inside, thick - mean, torch.zeros_like(thick)) ** 2).sum() / nf
    got = torch.cat((count.to(torch.float64), picked, torch.stack((mean, torch.sqrt(var))))).cpu().numpy()  # the one download
    if int(got[0]) == 0:
        return {'n': 0}
    return {'n': int(got[0]), 't2_max': float(got[1]), 't2_min': float(got[2]),
            'order': {v: (float(got[3 + 2 * k]), float(got[4 + 2 * k])) for k, v in enumerate(q)},
            'mean': float(got[-2]), 'std': float(got[-1])}
