"""Vessel territories on the device (csrc/territory.hip): which centreline voxel is nearest to every voxel of an organ,
the partition of the organ by nearest branch, and what hangs downstream of every branch of a rooted tree.

A renal arterial tree is extracted to answer which part of the kidney a branch feeds and how much of the kidney, and of
a tumour, falls when the branch is clamped; planning tools answer it with a nearest-branch (Voronoi) partition of the
parenchyma.  `nearest` is the exact Euclidean feature transform of a packed mask (the squared distances have the bits of
distance.edt_squared, the site is chosen by the tie rule of include/ru3d.h, "nearest site / territories"), `assign`
turns the nearest site into a label through the ids of `skeleton.graph`, `tally` counts labels against a second label
volume with integers only.  Their defining twins are transform._nearest_site_numpy, _site_assign_numpy and
_territory_tally_numpy.  Masks are `morphology.PackedMask`; there is no host fallback for these: every one of them wants
HIP tensors (the numpy route lives in transform.py and trainer.py).  `rooted` and `downstream` are host code on the small
tables and serve both routes.
"""
import ctypes

import numpy as np
import torch

import _native as N
from _native import check, ptr, stream
from distance import MAX_AXIS, _packed, _spacing


def _same_shape(mask, other, what):
    if other.shape != mask.shape or other.device != mask.device:
        raise ValueError("%s: operands of shape %s on %s and %s on %s" % (what, mask.shape, mask.device, tuple(other.shape),
                                                                          other.device))


def _volume(t, dtype, mask, what):
    if not torch.is_tensor(t) or t.dtype != dtype or tuple(t.shape) != mask.shape or t.device != mask.device:
        raise ValueError("%s must be a %s tensor of shape %s on %s" % (what, dtype, mask.shape, mask.device))
    return t.contiguous()


def nearest(sites, sampling=None, return_sq=True):
    """(index, sq): for every voxel the linear index (int32, into the volume of the mask's shape) of the nearest SET voxel
    of the PackedMask `sites` and the squared distance to it in `sampling` units (float64, the bits of
    distance.edt_squared; None with return_sq=False).  Equally near sites: the smaller coordinate wins pass by pass (z,
    y, x) - with a spacing whose products are exact, the smallest linear index.  No site at all: -1 and inf."""
    _packed(sites, "nearest")
    X, Y, Z = sites.shape3
    if X > MAX_AXIS or Y > MAX_AXIS:
        raise ValueError("nearest: a volume of shape %s is beyond the limit of %d voxels along every axis but the last"
                         % (sites.shape, MAX_AXIS))
    spacing = (ctypes.c_double * 3)(*_spacing(sampling, len(sites.shape)))
    index = torch.empty(sites.shape, dtype=torch.int32, device=sites.device)
    sq = torch.empty(sites.shape, dtype=torch.float64, device=sites.device) if return_sq else None
    # the transform's flag, and the values when the caller wants none back (include/ru3d.h)
    ws = N.workspace(N.lib.ru3d_edt_workspace_bytes(X, Y, Z) + (0 if return_sq else 8 * X * Y * Z), sites.device)
    N.note_device(sites.device)
    check(N.lib.ru3d_nearest_site(ptr(sites.bits), X, Y, Z, spacing, ptr(index), ptr(sq), ptr(ws), ws.numel(), stream()),
          "nearest_site")
    return index, sq


def assign(sites, site_ids, index, region=None):
    """int32 HIP volume: site_ids[rank] of the site `index` names, where the PackedMask `region` is set (None: everywhere)
    and index >= 0; 0 elsewhere.  site_ids is an int32 HIP vector over the set voxels of `sites` in element order - the
    order of distance.gather and of skeleton.graph's ids.  A vector of another length than the number of sites, or an
    index that is no site, raises."""
    _packed(sites, "assign")
    X, Y, Z = sites.shape3
    if region is not None:
        _packed(region, "assign")
        _same_shape(sites, region, "assign")
    index = _volume(index, torch.int32, sites, "assign: index")
    if (not torch.is_tensor(site_ids) or site_ids.dtype != torch.int32 or site_ids.dim() != 1
            or site_ids.device != sites.device):
        raise ValueError("assign: site_ids must be an int32 vector on %s" % sites.device)
    site_ids = site_ids.contiguous()
    labels = torch.empty(sites.shape, dtype=torch.int32, device=sites.device)
    ws = N.workspace(2 * N.lib.ru3d_skeleton_workspace_bytes(X, Y, Z), sites.device)
    N.note_device(sites.device)
    check(N.lib.ru3d_site_assign(ptr(sites.bits), None if region is None else ptr(region.bits), ptr(index),
                                 ptr(site_ids) if site_ids.numel() else None, site_ids.numel(), X, Y, Z, ptr(labels),
                                 ptr(ws), ws.numel(), stream()), "site_assign")
    return labels


def tally(labels, K, other=None, num_other=0, region=None):
    """int64 HIP tensor [K + 1, num_other + 1]: the voxels of the PackedMask `region` (None: all) per label 0 .. K of the
    int32 HIP volume `labels` and per value min(other, num_other) of the uint8 HIP volume `other` (None: one column).
    Row 0 is the region's voxels without a site.  A label outside 0 .. K raises."""
    if not torch.is_tensor(labels) or labels.dtype != torch.int32 or not 1 <= labels.dim() <= 3:
        raise ValueError("tally: labels must be an int32 tensor of 1 to 3 axes")
    N.require_device(labels, "tally: labels")
    if int(K) != K or K < 0 or int(num_other) != num_other or not 0 <= num_other <= 255 or (other is None and num_other):
        raise ValueError("tally: K=%r, num_other=%r (K >= 0, 0 <= num_other <= 255, 0 without `other`)" % (K, num_other))
    shape = tuple(labels.shape)
    X, Y, Z = (1,) * (3 - len(shape)) + shape
    labels = labels.contiguous()
    if region is not None:
        _packed(region, "tally")
        _same_shape(region, labels, "tally")
    if other is not None:
        if not torch.is_tensor(other) or other.dtype != torch.uint8 or tuple(other.shape) != shape or other.device != labels.device:
            raise ValueError("tally: other must be a uint8 tensor of shape %s on %s" % (shape, labels.device))
        other = other.contiguous()
    table = torch.empty((int(K) + 1, int(num_other) + 1), dtype=torch.int64, device=labels.device)
    ws = N.workspace(256, labels.device)
    N.note_device(labels.device)
    check(N.lib.ru3d_territory_tally(ptr(labels), int(K), ptr(other), int(num_other),
                                     None if region is None else ptr(region.bits), X, Y, Z, ptr(table), ptr(ws),
                                     ws.numel(), stream()), "territory_tally")
    return table


def branch_sites(g):
    """(site_ids, K): the ids of a graph (skeleton.graph or its numpy twin: +b on a voxel of branch b, -m on a voxel of
    node m) as positive site ids - branch b stays b, node m becomes B + m - and K = B + M."""
    ids, B = g['ids'], int(g['branches'])
    if torch.is_tensor(ids):
        return torch.where(ids > 0, ids, B - ids).to(torch.int32), B + int(g['nodes'])
    return np.where(ids > 0, ids, B - ids).astype(np.int32), B + int(g['nodes'])


METRICS = ('euclidean', 'geodesic')
# the steps of the geodesic metric: all 26, so that a path may cut a corner as a straight line does
GEODESIC_STRUCTURE = np.ones((3, 3, 3), dtype=bool)


def check_metric(metric, what):
    if metric not in METRICS:
        raise ValueError("%s: metric=%r (one of %s)" % (what, metric, ', '.join(repr(m) for m in METRICS)))
    return metric


def partition(skel, g, region, sampling=None, other=None, num_other=0, metric='euclidean', vessel=None):
    """(table, labels): the voxels of the PackedMask `region` by nearest voxel of the skeleton `skel` whose graph is `g`
    (skeleton.graph(skel, ...)).  labels is the int32 HIP volume of territories (branch b -> b, node m -> B + m, 0
    outside the region), table the host int64 [B + M + 1, num_other + 1] tally of them against `other`.  Only the table
    is downloaded.  metric='euclidean': nearest in a straight line (`nearest`).  metric='geodesic': nearest along a
    path of 26-neighbour steps that stays inside the region united with the PackedMask `vessel` (the lumen the skeleton
    lies in; required) - geodesic.grow from the skeleton voxels as seeds, each carrying its id; a region voxel that no
    such path reaches has label 0 and counts in row 0."""
    check_metric(metric, "partition")
    site_ids, K = branch_sites(g)
    if metric == 'geodesic':
        import geodesic
        import morphology
        _packed(skel, "partition")
        _packed(region, "partition")
        if vessel is None:
            raise ValueError("partition: metric='geodesic' needs the vessel mask the skeleton lies in (vessel=)")
        _packed(vessel, "partition")
        _same_shape(skel, region, "partition")
        _same_shape(skel, vessel, "partition")
        seeds = torch.zeros(skel.shape, dtype=torch.int32, device=skel.device)
        seeds[morphology.unpack(skel) != 0] = site_ids                      # element order: the order of the ids
        allowed = morphology.PackedMask(region.bits | vessel.bits, region.shape)
        _, reached = geodesic.grow(seeds, allowed, sampling, GEODESIC_STRUCTURE[(1,) * (3 - len(skel.shape))])
        labels = torch.where(morphology.unpack(region) != 0, reached, torch.zeros_like(reached))
    else:
        index, _ = nearest(skel, sampling, return_sq=False)
        labels = assign(skel, site_ids, index, region)
    return tally(labels, K, other, num_other, region).cpu().numpy(), labels


# ------------------------------------------------------------------ the rooted tree (host code, both routes)
def rooted(node_table, branch_table, radius_mean, root=None):
    """The graph of skeleton.graph read as a tree from a root node.  root=None picks the ostium: the node of valence 1
    whose branch has the largest mean radius, the smallest node number on a tie; otherwise `root` is a node number
    (1 .. M).  Breadth-first from the root, nodes first in first out, a node's branches in increasing id.  A dict:
      root        the root's node number (0 when the graph has no node of valence 1 and none was given),
      parent      int64 [B]: the branch through which a branch is reached, 0 for a branch at the root,
      depth       int64 [B]: 0 at the root's branches, parent's depth + 1 below; -1 where unreachable,
      order       int64 [B]: the Strahler order on the tree (1 at a leaf; the largest order of the children, plus one
                  when two or more children have it); 0 where unreachable or a chord,
      reachable   bool [B]: the branch hangs on the root's component (loops without nodes and other components do not),
      chord       bool [B]: the branch was met when both its nodes had been reached: it closes a cycle and carries nothing
                  downstream; its parent is the branch that reached the node it was met from, and it counts for no
                  Strahler order,
      far         int64 [B]: the node a tree branch leads to (0 for a chord or an unreachable branch)."""
    node_table, branch_table = np.asarray(node_table), np.asarray(branch_table)
    M, B = len(node_table), len(branch_table)
    radius_mean = np.asarray(radius_mean, dtype=np.float64)
    parent, depth, order = np.zeros(B, np.int64), np.full(B, -1, np.int64), np.zeros(B, np.int64)
    reachable, chord, far = np.zeros(B, bool), np.zeros(B, bool), np.zeros(B, np.int64)
    out = {'root': 0, 'parent': parent, 'depth': depth, 'order': order, 'reachable': reachable, 'chord': chord, 'far': far}
    at = [[] for _ in range(M + 1)]                                          # node -> its branches in increasing id
    for b in range(B):
        n0, n1 = int(branch_table[b, 3]), int(branch_table[b, 4])
        if n0 >= 1:
            at[n0].append(b + 1)
            if n1 != n0:
                at[n1].append(b + 1)
    if root is None:
        best = None
        for m in range(1, M + 1):
            if node_table[m - 1, 1] == 1 and len(at[m]) == 1:
                r = radius_mean[at[m][0] - 1]
                if best is None or r > best[0]:                             # nan never wins: a radius is needed
                    best = (r, m)
        if best is None:
            return out
        root = best[1]
    elif int(root) != root or not 1 <= root <= M:
        raise ValueError("rooted: root=%r (None or a node number 1 .. %d)" % (root, M))
    root = int(root)
    out['root'] = root
    reached = np.zeros(M + 1, bool)
    reached[root] = True
    via = np.zeros(M + 1, np.int64)                                         # node -> the branch that reached it
    queue, children, visited = [root], [[] for _ in range(B + 1)], []
    while queue:
        m = queue.pop(0)
        for b in at[m]:
            if reachable[b - 1]:
                continue
            reachable[b - 1] = True
            n0, n1 = int(branch_table[b - 1, 3]), int(branch_table[b - 1, 4])
            other = n1 if n0 == m else n0
            parent[b - 1] = via[m]
            depth[b - 1] = depth[via[m] - 1] + 1 if via[m] else 0
            if reached[other]:                                              # the same node twice, or a node met before
                chord[b - 1] = True
                continue
            reached[other] = True
            via[other] = b
            far[b - 1] = other
            children[via[m]].append(b)
            visited.append(b)
            queue.append(other)
    for b in reversed(visited):                                             # children before their parent
        orders = [order[c - 1] for c in children[b]]
        top = max(orders, default=0)
        order[b - 1] = 1 if not orders else top + (1 if orders.count(top) >= 2 else 0)
    return out


def downstream(table, tree, B):
    """int64 [B, columns]: per branch the rows of `table` (tally's: row b for branch b, row B + m for node m) of the
    branch itself, of the node it leads to and of everything beyond that node in the tree `tree` (rooted).  A node's
    territory goes with the branch that reaches it; the root node's goes to the first branch at the root.  A chord or an
    unreachable branch has its own row alone; a chord's row is part of its parent's sum, once, so the branch at the root
    sums every reachable row."""
    table = np.asarray(table, dtype=np.int64)
    B = int(B)
    total = table[1:B + 1].copy()
    parent, depth, far = tree['parent'], tree['depth'], tree['far']
    tree_branches = [b for b in range(1, B + 1) if far[b - 1] > 0]
    for b in tree_branches:
        total[b - 1] += table[B + far[b - 1]]
    at_root = [b for b in tree_branches if parent[b - 1] == 0]
    if at_root:
        total[at_root[0] - 1] += table[B + tree['root']]
    hanging = [b for b in range(1, B + 1) if tree['reachable'][b - 1]]       # tree branches and chords
    for b in sorted(hanging, key=lambda b: -depth[b - 1]):                  # deepest first: sums are complete when passed up
        if parent[b - 1]:
            total[parent[b - 1] - 1] += total[b - 1]
    return total
