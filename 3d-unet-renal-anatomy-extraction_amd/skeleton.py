"""Curve skeletons of packed masks on the device (csrc/skeleton.hip): a topology-preserving 3D thinning, end and
junction voxels, the length of the voxel graph, the overlap counts of centreline Dice and the radii along a centreline.

Overlap Dice and surface distances say little about a thin tubular structure; what the anatomy's arteries and veins
are judged by is centreline Dice, and what is wanted from an extracted tree is its centreline, radii and branch points.
All of it hangs on a curve skeleton.  The thinning's contract is written down in include/ru3d.h ("skeleton") and its
defining twin is `transform._skeleton_numpy`: the device result equals it voxel for voxel.  Masks are
`morphology.PackedMask`.  There is no host fallback in here: every function wants HIP tensors (the numpy route lives in
transform.py and trainer.py).
"""
import ctypes
import math

import torch

import _native as N
import distance
from _native import check, ptr, stream
from distance import _packed, _spacing
from morphology import PackedMask


def _same(a, b, what):
    _packed(a, what)
    _packed(b, what)
    if a.shape != b.shape or a.device != b.device:
        raise ValueError("%s: masks of shape %s on %s and %s on %s" % (what, a.shape, a.device, b.shape, b.device))


def thin(mask, max_iterations=None, return_iterations=False):
    """The curve skeleton of a PackedMask as a new PackedMask; `mask` is left as it is.  max_iterations=None thins until
    a whole iteration deletes nothing.  One host read per iteration (the deletion counter), nothing else leaves the
    device.  return_iterations=True returns (skeleton, iterations run), the last, idle iteration included."""
    _packed(mask, "thin")
    if max_iterations is not None and (int(max_iterations) != max_iterations or max_iterations < 0):
        raise ValueError("thin: max_iterations=%r (None or a count >= 0)" % (max_iterations,))
    X, Y, Z = mask.shape3
    out = PackedMask(mask.bits.clone(), mask.shape)
    ws = N.workspace(N.lib.ru3d_skeleton_workspace_bytes(X, Y, Z), mask.device)
    N.note_device(mask.device)
    rc = N.lib.ru3d_skeleton_thin(ptr(out.bits), X, Y, Z, -1 if max_iterations is None else int(max_iterations), ptr(ws),
                                  ws.numel(), stream())
    if rc < 0:
        check(rc, "skeleton_thin")
    return (out, rc) if return_iterations else out


def classify(skel):
    """(ends, junctions, n_voxels, n_ends, n_junctions): PackedMasks of the voxels with exactly one and with three or
    more set voxels among their 26 neighbours, and the three counts as Python ints (one download)."""
    _packed(skel, "classify")
    X, Y, Z = skel.shape3
    ends, junctions = skel.new(), skel.new()
    counts = torch.empty(3, dtype=torch.int64, device=skel.device)
    N.note_device(skel.device)
    check(N.lib.ru3d_skeleton_classify(ptr(skel.bits), X, Y, Z, ptr(ends.bits), ptr(junctions.bits), ptr(counts), stream()),
          "skeleton_classify")
    n, n_ends, n_junctions = (int(c) for c in counts.tolist())
    return ends, junctions, n, n_ends, n_junctions


def length_device(skel, sampling=None):
    """float64 HIP tensor [1]: `length` without the host read."""
    _packed(skel, "length")
    X, Y, Z = skel.shape3
    spacing = (ctypes.c_double * 3)(*_spacing(sampling, len(skel.shape)))
    out = torch.empty(1, dtype=torch.float64, device=skel.device)
    ws = N.workspace(256, skel.device)
    N.note_device(skel.device)
    check(N.lib.ru3d_skeleton_length(ptr(skel.bits), X, Y, Z, spacing, ptr(out), ptr(ws), ws.numel(), stream()),
          "skeleton_length")
    return out


def length(skel, sampling=None):
    """The length of the skeleton's voxel graph in `sampling` units (None: voxels): the sum, over the unordered pairs of
    26-adjacent set voxels, of the distance between their centres, in float64 with a fixed order (include/ru3d.h), so
    it equals the numpy route with ==.  Every edge of the graph counts, the short diagonals inside the clique of voxels
    at a junction too: exact for a curve without junctions, a few voxel steps long at each branch point."""
    return float(length_device(skel, sampling).item())


def overlap_device(a, b):
    """int64 HIP tensor [3]: `overlap` without the host read."""
    _same(a, b, "overlap")
    X, Y, Z = a.shape3
    counts = torch.empty(3, dtype=torch.int64, device=a.device)
    N.note_device(a.device)
    check(N.lib.ru3d_skeleton_overlap(ptr(a.bits), ptr(b.bits), X, Y, Z, ptr(counts), stream()), "skeleton_overlap")
    return counts


def overlap(a, b):
    """(|a|, |b|, |a & b|) of two PackedMasks of one shape as Python ints."""
    return tuple(int(c) for c in overlap_device(a, b).tolist())


def complement(mask):
    """The unset voxels of a PackedMask as a new PackedMask; the padding bits at z >= Z stay 0."""
    _packed(mask, "complement")
    bits = torch.bitwise_not(mask.bits)
    Z = mask.shape3[2]
    if Z & 63:
        bits[..., -1] &= (1 << (Z & 63)) - 1
    return PackedMask(bits, mask.shape)


def radii_squared(skel, mask, sampling=None):
    """float64 HIP vector: the squared distance, in `sampling` units, from every voxel of `skel` (element order) to the
    nearest voxel outside `mask` - the exact transform of distance.edt_squared on the packed complement, gathered with
    distance.gather."""
    _same(skel, mask, "radii")
    return distance.gather(distance.edt_squared(complement(mask), sampling), skel)


def radius_stats(sq):
    """(n, min, mean, max) of the radii whose squares are the float64 HIP vector `sq`; the mean's sum has the fixed
    order of include/ru3d.h.  n == 0 gives (0, nan, nan, nan).  One download of four numbers."""
    if not torch.is_tensor(sq) or sq.dtype != torch.float64 or sq.dim() != 1 or not sq.is_contiguous():
        raise ValueError("radius_stats: sq must be a contiguous float64 vector")
    N.require_device(sq, "radius_stats")
    out = torch.empty(4, dtype=torch.float64, device=sq.device)
    check(N.lib.ru3d_skeleton_radius_stats(ptr(sq) if sq.numel() else None, sq.numel(), ptr(out), stream()),
          "skeleton_radius_stats")
    n, lo, hi, total = out.tolist()
    if not n:
        return 0, float('nan'), float('nan'), float('nan')
    return int(n), math.sqrt(lo), total / n, math.sqrt(hi)


def radii(skel, mask, sampling=None):
    """(min, mean, max) radius along a skeleton, in `sampling` units (millimetres with the voxel spacing): the distance
    from each skeleton voxel to the nearest voxel outside `mask`.  Where the object touches a face of the volume the
    transform sees no background beyond that face, as scipy.ndimage.distance_transform_edt does not: radii there are
    measured to the nearest background voxel inside the volume, and a mask without any background voxel gives inf.
    An empty skeleton gives nan."""
    return radius_stats(radii_squared(skel, mask, sampling))[1:]
