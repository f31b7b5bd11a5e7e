"""Triangle meshes of packed masks on the device (csrc/mesh.hip): the faces between a set voxel and an unset one, the
lattice edge graph of their corners, Taubin smoothing on that graph, area / enclosed volume and the voxel-to-world map.

The contract (vertex, quad and triangle order, the smoothing expression, the sums) is written down in include/ru3d.h
and restated in numpy by `transform.extract_mesh`; integer outputs and smoothed positions of the two routes are equal
with `==`.  Masks are `morphology.PackedMask`, or a uint8 / bool HIP volume that is packed here (`!= 0`).  There is no
host fallback in here: every function wants HIP tensors.
"""
import numpy as np
import torch

import _native as N
from _native import check, ptr, stream
from morphology import PackedMask, pack

MAX_VERTICES = 1 << 31                  # V and 2 Q stay below it (int32 vertex numbers and face rows)


class Mesh:
    """`corners` int32 [V, 3] lattice corners, `vertices` float64 [V, 3] positions in voxel coordinates (corners - 0.5
    until smoothed), `faces` int32 [2 Q, 3] vertex numbers, `neighbours` int32 [V, 6] edge graph (-1: none), `shape` the
    shape of the volume.  numpy arrays on the host route, HIP tensors on the device route."""

    def __init__(self, corners, vertices, faces, neighbours, shape):
        self.corners = corners
        self.vertices = vertices
        self.faces = faces
        self.neighbours = neighbours
        self.shape = tuple(int(s) for s in shape)


def _as_packed(mask, what):
    if isinstance(mask, PackedMask):
        N.require_device(mask.bits, what)
        return mask
    if torch.is_tensor(mask):
        return pack(mask)
    raise ValueError("%s: expected a PackedMask (morphology.pack) or a uint8 / bool HIP volume, got %s"
                     % (what, type(mask).__name__))


def count(mask):
    """(V, Q) of a PackedMask or a uint8 / bool HIP volume as Python ints: one host read."""
    mask = _as_packed(mask, "count")
    X, Y, Z = mask.shape3
    counts = torch.empty(2, dtype=torch.int64, device=mask.device)
    ws = N.workspace(N.lib.ru3d_mesh_workspace_bytes(X, Y, Z), mask.device)
    N.note_device(mask.device)
    check(N.lib.ru3d_mesh_count(ptr(mask.bits), X, Y, Z, ptr(counts), ptr(ws), ws.numel(), stream()), "mesh_count")
    V, Q = (int(c) for c in counts.tolist())
    return V, Q


def extract(mask):
    """The unsmoothed surface of a PackedMask or a uint8 / bool HIP volume (1 to 3 axes) as a Mesh of HIP tensors.
    The two counts are read back once, between the counting pass and the pass that fills buffers of exactly that size."""
    mask = _as_packed(mask, "extract")
    X, Y, Z = mask.shape3
    device = mask.device
    V, Q = count(mask)
    if V >= MAX_VERTICES or 2 * Q >= MAX_VERTICES:
        raise ValueError("extract: a surface of %d vertices and %d triangles is beyond the limit of 2**31 - 1 each"
                         % (V, 2 * Q))
    corners = torch.empty((V, 3), dtype=torch.int32, device=device)
    neighbours = torch.empty((V, 6), dtype=torch.int32, device=device)
    faces = torch.empty((2 * Q, 3), dtype=torch.int32, device=device)
    if V or Q:
        counts = torch.empty(2, dtype=torch.int64, device=device)
        ws = N.workspace(N.lib.ru3d_mesh_workspace_bytes(X, Y, Z), device)
        N.note_device(device)
        check(N.lib.ru3d_mesh_emit(ptr(mask.bits), X, Y, Z, ptr(corners) if V else None, ptr(neighbours) if V else None,
                                   V, ptr(faces) if Q else None, Q, ptr(counts), ptr(ws), ws.numel(), stream()),
              "mesh_emit")
    return Mesh(corners, corners.to(torch.float64) - 0.5, faces, neighbours, mask.shape)


def _positions(vertices, what):
    if (not torch.is_tensor(vertices) or vertices.dtype != torch.float64 or vertices.dim() != 2
            or vertices.shape[1] != 3):
        raise ValueError("%s: vertices must be a float64 tensor [V, 3]" % what)
    N.require_device(vertices, "%s: vertices" % what)
    return vertices.contiguous()


def _table(t, columns, device, what, name):
    if (not torch.is_tensor(t) or t.dtype != torch.int32 or t.dim() != 2 or t.shape[1] != columns
            or t.device != device):
        raise ValueError("%s: %s must be an int32 tensor [n, %d] on %s" % (what, name, columns, device))
    return t.contiguous()


def umbrella(vertices, neighbours, factor):
    """One umbrella step as a new tensor: q[v] = p[v] + factor * (mean of the present neighbours - p[v])."""
    src = _positions(vertices, "umbrella")
    nb = _table(neighbours, 6, src.device, "umbrella", "neighbours")
    if nb.shape[0] != src.shape[0]:
        raise ValueError("umbrella: %d rows of neighbours for %d vertices" % (nb.shape[0], src.shape[0]))
    dst = torch.empty_like(src)
    if src.shape[0]:
        N.note_device(src.device)
        check(N.lib.ru3d_mesh_smooth(ptr(src), ptr(dst), ptr(nb), src.shape[0], float(factor), stream()), "mesh_smooth")
    return dst


def smooth(m, iterations=10, lam=0.5, mu=-0.53):
    """Taubin smoothing of a Mesh: `iterations` times (umbrella step with lam, then with mu), ping-ponging between two
    buffers, one launch per half step.  Returns a Mesh that shares everything but `vertices` with `m`;
    iterations=0 returns the input positions."""
    if int(iterations) != iterations or iterations < 0:
        raise ValueError("smooth: iterations=%r (a count >= 0)" % (iterations,))
    p = _positions(m.vertices, "smooth")
    for _ in range(int(iterations)):
        p = umbrella(umbrella(p, m.neighbours, lam), m.neighbours, mu)
    return Mesh(m.corners, p, m.faces, m.neighbours, m.shape)


def measure(vertices, faces):
    """float64 HIP tensor [2]: (area, enclosed volume) of the triangles `faces` over the positions `vertices`, in the
    units of the positions.  Fixed partition and trees: the same bits in every run.  No host read."""
    v = _positions(vertices, "measure")
    f = _table(faces, 3, v.device, "measure", "faces")
    out = torch.zeros(2, dtype=torch.float64, device=v.device)
    if v.shape[0] and f.shape[0]:
        ws = N.workspace(N.lib.ru3d_mesh_measure_workspace_bytes(f.shape[0]), v.device)
        N.note_device(v.device)
        check(N.lib.ru3d_mesh_measure(ptr(v), v.shape[0], ptr(f), f.shape[0], ptr(out), ptr(ws), ws.numel(), stream()),
              "mesh_measure")
    return out


def world_terms(affine):
    """(rotation-and-zoom part [3, 3], translation [3], True when the map turns the orientation over) of a 4 x 4
    voxel-to-world affine, as float64 numpy."""
    a = np.asarray(affine, dtype=np.float64)
    if a.shape != (4, 4):
        raise ValueError("affine: expected a 4 x 4 matrix, got shape %s" % (a.shape,))
    return a[:3, :3], a[:3, 3], bool(np.linalg.det(a[:3, :3]) < 0)


def to_world(vertices, affine, faces=None):
    """`vertices @ A[:3, :3].T + A[:3, 3]` in float64, spelled per column so that numpy and torch round alike.  With
    `faces` given, returns (positions, faces) and swaps the faces' last two columns when det(A[:3, :3]) < 0: normals
    still point outward and the signed volume stays positive."""
    v = _positions(vertices, "to_world")
    r, t, flipped = world_terms(affine)
    cols = [v[:, 0:1] * torch.as_tensor(r[:, 0], device=v.device), v[:, 1:2] * torch.as_tensor(r[:, 1], device=v.device),
            v[:, 2:3] * torch.as_tensor(r[:, 2], device=v.device)]
    out = cols[0] + cols[1] + cols[2] + torch.as_tensor(t, device=v.device)
    if faces is None:
        return out
    return out, (faces[:, [0, 2, 1]].contiguous() if flipped else faces)
