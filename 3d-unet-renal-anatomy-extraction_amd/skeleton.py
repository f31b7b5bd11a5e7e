"""Curve skeletons of packed masks on the device (csrc/skeleton.hip): a topology-preserving 3D thinning, end and
junction voxels, the length of the voxel graph, the overlap counts of centreline Dice and the radii along a centreline.

Overlap Dice and surface distances say little about a thin tubular structure; what the anatomy's arteries and veins
are judged by is centreline Dice, and what is wanted from an extracted tree is its centreline, radii and branch points.
All of it hangs on a curve skeleton.  The thinning's contract is written down in include/ru3d.h ("skeleton") and its
defining twin is `transform._skeleton_numpy`: the device result equals it voxel for voxel.  `graph` and `prune`
(csrc/skeleton_graph.hip; contract "skeleton graph", twin `transform._skeleton_graph_numpy`) read a skeleton as nodes and
branches - segments, what they hang on, their lengths and radii - and remove the spurs of the thinning.  Masks are
`morphology.PackedMask`.  There is no host fallback in here: every function wants HIP tensors (the numpy route lives in
transform.py and trainer.py).
"""
import ctypes
import math

import numpy as np
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


# ------------------------------------------------------------------ the voxel graph: nodes, branches, pruning
_IDS_INITIAL_CAPACITY = 1 << 20         # set voxels the ids buffer holds before it has to grow
_ids_capacity = {}                      # device -> ids per buffer
_Q = float(1 << 24)                     # the fixed point of rsum_q (include/ru3d.h)


def _graph_workspace(skel):
    """The scratch of the three graph entry points: three times the thinning's (include/ru3d.h)."""
    X, Y, Z = skel.shape3
    return N.workspace(3 * N.lib.ru3d_skeleton_workspace_bytes(X, Y, Z), skel.device)


def _graph_label(skel):
    """(ids, n, M, B): one labelling of the skeleton's voxel graph and the one host read of its three counts.  The ids
    buffer has a remembered capacity; a mask with more set voxels grows it and is labelled once more."""
    X, Y, Z = skel.shape3
    device = skel.device
    ws = _graph_workspace(skel)
    counts = torch.empty(3, dtype=torch.int64, device=device)
    N.note_device(device)
    while True:
        cap = min(_ids_capacity.get(device, _IDS_INITIAL_CAPACITY), X * Y * Z)
        ids = torch.empty(cap, dtype=torch.int32, device=device)
        check(N.lib.ru3d_skeleton_graph_label(ptr(skel.bits), X, Y, Z, ptr(ids), cap, ptr(counts), ptr(ws), ws.numel(), stream()),
              "skeleton_graph_label")
        n, nodes, branches = (int(c) for c in counts.tolist())
        if n <= cap:
            return ids[:n], n, nodes, branches
        _ids_capacity[device] = 1 << (n - 1).bit_length()


def _step_lengths(spacing):
    """The 13 step lengths of ru3d_skeleton_length: sqrt(fl(A + fl(B + C))), A = fl(fl(sx dx)^2), cells 14 .. 26."""
    sx, sy, sz = spacing
    steps = []
    for cell in range(14, 27):
        ax, ay, az = sx * (cell // 9 - 1), sy * ((cell // 3) % 3 - 1), sz * (cell % 3 - 1)
        steps.append(math.sqrt(ax * ax + (ay * ay + az * az)))
    return steps


def graph(skel, mask=None, sampling=None):
    """The voxel graph of a PackedMask (a curve skeleton; any mask will do) as nodes and branches - the contract of
    include/ru3d.h, "skeleton graph", whose defining twin is transform._skeleton_graph_numpy.  A dict:
      ids            int32 HIP vector over the set voxels in element order (the order of distance.gather): +b on a voxel
                     of branch b, -m on a voxel of node m,
      n, nodes, branches   the numbers of set voxels, of nodes (M) and of branches (B),
      node_table     host int64 [M, 6]: voxels, valence, sum_x, sum_y, sum_z, first,
      branch_table   host int64 [B, 18]: voxels, t0, t1, n0, n1, pairs[13],
      length         float64 [B] in `sampling` units, folded from the pairs in the order of skeleton.length,
      chord          float64 [B], the distance between the two terminal voxels (nan for a loop),
      tortuosity     length / chord (nan where the chord is 0 or nan),
    and with `mask`, the PackedMask the radii are measured in (skeleton.radii_squared), per branch over its path voxels
      radius_min, radius_mean, radius_max   float64 [B]; the mean is inf when a radius is.
    Two host reads: the three counts that size the tables, and the tables."""
    _packed(skel, "graph")
    if mask is not None:
        _same(skel, mask, "graph")
    X, Y, Z = skel.shape3
    spacing = _spacing(sampling, len(skel.shape))
    device = skel.device
    radii_volume = None
    if mask is not None:
        radii_volume = distance.edt_squared(complement(mask), sampling).contiguous()
    ids, n, M, B = _graph_label(skel)
    table = torch.empty(M * 6 + B * 18 + (B * 3 if mask is not None else 0), dtype=torch.int64, device=device)
    nodes, branches, radii = table[:M * 6], table[M * 6:M * 6 + B * 18], table[M * 6 + B * 18:]
    ws = _graph_workspace(skel)
    N.note_device(device)
    with_radii = mask is not None and B > 0
    check(N.lib.ru3d_skeleton_graph_measure(ptr(skel.bits), X, Y, Z, ptr(ids) if n else None, n, M, B,
                                            ptr(radii_volume) if with_radii else None, ptr(nodes) if M else None,
                                            ptr(branches) if B else None, ptr(radii) if with_radii else None, ptr(ws),
                                            ws.numel(), stream()), "skeleton_graph_measure")
    host = table.cpu().numpy()                                             # the second host read
    node_table = host[:M * 6].reshape(M, 6).copy()
    branch_table = host[M * 6:M * 6 + B * 18].reshape(B, 18).copy()
    out = {'ids': ids, 'n': n, 'nodes': M, 'branches': B, 'node_table': node_table, 'branch_table': branch_table}
    length = np.zeros(B, dtype=np.float64)
    for k, step in enumerate(_step_lengths(spacing)):
        length = length + branch_table[:, 5 + k].astype(np.float64) * step
    t0, t1 = branch_table[:, 1], branch_table[:, 2]
    open_ = t0 >= 0
    legs = []
    for s, a0, a1 in zip(spacing, np.unravel_index(np.where(open_, t0, 0), (X, Y, Z)),
                         np.unravel_index(np.where(open_, t1, 0), (X, Y, Z))):
        d = s * (a1 - a0).astype(np.float64)
        legs.append(d * d)
    chord = np.where(open_, np.sqrt(legs[0] + (legs[1] + legs[2])), np.nan)
    with np.errstate(divide='ignore', invalid='ignore'):
        tortuosity = np.where(chord > 0, length / chord, np.nan)
    out.update(length=length, chord=chord, tortuosity=tortuosity)
    if mask is not None:
        cols = host[M * 6 + B * 18:].reshape(B, 3)
        rmin_sq, rmax_sq, rsum_q = cols[:, 0].copy().view(np.float64), cols[:, 1].copy().view(np.float64), cols[:, 2]
        with np.errstate(divide='ignore', invalid='ignore'):
            mean = rsum_q.astype(np.float64) / _Q / branch_table[:, 0].astype(np.float64)
        out.update(radius_min=np.sqrt(rmin_sq), radius_mean=np.where(np.isinf(rmax_sq), np.inf, mean),
                   radius_max=np.sqrt(rmax_sq))
    return out


def spurs(node_table, branch_table, length, min_length):
    """(branch flags [B], node flags [M], both bool) of the spurs of a graph: a branch shorter than min_length with
    exactly one end on a node of valence 1 made of a single voxel and the other end on a node of valence >= 3; the
    flagged nodes are those single end voxels."""
    B, M = len(branch_table), len(node_table)
    kill_branch, kill_node = np.zeros(B, dtype=bool), np.zeros(M, dtype=bool)
    if not B or not M:
        return kill_branch, kill_node
    n0, n1 = branch_table[:, 3], branch_table[:, 4]
    open_ = n0 >= 1
    a, b = np.where(open_, n0, 1) - 1, np.where(open_, n1, 1) - 1
    leaf = (node_table[:, 1] == 1) & (node_table[:, 0] == 1)
    fork = node_table[:, 1] >= 3
    tip_a, tip_b = leaf[a] & fork[b], leaf[b] & fork[a]
    kill_branch = open_ & (tip_a ^ tip_b) & (length < min_length)
    kill_node[a[kill_branch & tip_a]] = True
    kill_node[b[kill_branch & tip_b]] = True
    return kill_branch, kill_node


def prune(skel, min_length, sampling=None, max_rounds=None):
    """(new PackedMask, rounds): `skel` without its spurs (see `spurs`; lengths in `sampling` units); `skel` is left as it
    is.  A round erases the path voxels and the end voxel of every spur of the graph as it is when the round begins,
    then the graph is analysed again; rounds repeat until one finds no spur (that round is counted) or max_rounds.
    Junction voxels are never erased, so pruning disconnects nothing.  The twin is transform._skeleton_prune_numpy."""
    _packed(skel, "prune")
    if max_rounds is not None and (int(max_rounds) != max_rounds or max_rounds < 0):
        raise ValueError("prune: max_rounds=%r (None or a count >= 0)" % (max_rounds,))
    if not float(min_length) >= 0:
        raise ValueError("prune: min_length=%r (>= 0)" % (min_length,))
    X, Y, Z = skel.shape3
    out = PackedMask(skel.bits.clone(), skel.shape)
    rounds = 0
    while max_rounds is None or rounds < max_rounds:
        g = graph(out, sampling=sampling)
        rounds += 1
        kill_branch, kill_node = spurs(g['node_table'], g['branch_table'], g['length'], float(min_length))
        if not kill_branch.any():
            break
        flags = torch.from_numpy(np.concatenate((kill_branch, kill_node)).astype(np.uint8)).to(out.device)
        ws = _graph_workspace(out)
        N.note_device(out.device)
        check(N.lib.ru3d_skeleton_graph_erase(ptr(out.bits), X, Y, Z, ptr(g['ids']), g['n'], g['nodes'], g['branches'],
                                              ptr(flags[:g['branches']]), ptr(flags[g['branches']:]), ptr(ws), ws.numel(),
                                              stream()), "skeleton_graph_erase")
    return out, rounds
