"""Drop-in `transform` module: the reference's case transforms (reference transform.py) for host-side DataLoader
workers, plus the on-device pipeline (`DeviceAugment`, augment.py) that replaces them when the cases live in HBM.

Every class / function of the reference module that the training and inference scripts import is here under its
name and with its arguments (nb_train_iia.py:8-10, data.py:1-2, trainer.py:8): rescale, resize, crop_pad_to_bbox,
pad, crop_pad, to_tensor / to_numpy, to_one_hot, combination_labels, remove_small_region and the Random* / Crop* /
To* classes; `Compose` stands in for torchvision's (absent here).  Cases are dicts with a channels-last float32
'image' [d1, d2, d3, C] and an integer 'label' [d1, d2, d3]; the interpolation is scipy.ndimage.zoom exactly as in the
reference (third-party there too).  The random draws come from numpy's global generator in the reference's order, so a
seed reproduces the reference's patches (checked against tests/golden/g7_augment.npz).
"""
import math

import numpy as np
import scipy.ndimage as ndi
import torch

from augment import DeviceAugment, DeviceCase  # noqa: F401  (the on-device replacement of the Random* chain)
import degrade
import locations
import spatial
from locations import class_locations  # noqa: F401  (the numpy twin of ru3d_class_index)
from spatial import bspline_displacement, resample_at, rotation_matrix, spatial_coordinates  # noqa: F401


class Compose(object):
    """torchvision.transforms.Compose as the scripts use it (nb_train_iia.py:30)."""

    def __init__(self, transforms):
        self.transforms = list(transforms)

    def __call__(self, case):
        for t in self.transforms:
            case = t(case)
        return case


def _as_range(v):
    if isinstance(v, float):
        assert 0 <= v <= 1, "If range is a single number, it must be non negative"
        return [1 - v, 1 + v]
    return v


def _per_axis(v, dim):
    return list(v) if isinstance(v, (np.ndarray, tuple, list)) else [v] * dim


# ------------------------------------------------------------------ layout helpers (transform.py:23-30, 144-173)
def split_dim(input, axis=-1):
    return [np.squeeze(a, axis=axis) for a in np.split(input, input.shape[axis], axis=axis)]


def slice_dim(input, slice, axis=-1):
    return split_dim(input, axis=axis)[slice]


def to_tensor(input):
    """(d1, ..., dn, C) -> (C, d1, ..., dn)"""
    return np.moveaxis(input, -1, 0)


def to_numpy(input):
    """(C, d1, ..., dn) -> (d1, ..., dn, C)"""
    return np.moveaxis(input, 0, -1)


def to_one_hot(input, num_classes, to_tensor=False):
    """transform.py:262-276: labels -> one-hot in the label's dtype, class axis last (or first)."""
    onehot = np.eye(num_classes)[input]
    if to_tensor:
        onehot = np.moveaxis(onehot, -1, 0)
    return onehot.astype(input.dtype)


# ------------------------------------------------------------------ resampling (transform.py:32-101)
def _zoom(a, scale, order, mode, cval):
    return ndi.zoom(a.astype(np.float32), scale, order=order, mode=mode, cval=cval)


def rescale(input, scale, order=1, mode='reflect', cval=0, is_label=False, multi_class=False):
    """scipy.ndimage.zoom with label support: labels with three or more classes present are interpolated per class
    (one-hot) and arg-maxed; fewer classes (or order 0) go through zoom directly and are cast back."""
    dtype = input.dtype
    if is_label:
        num_classes = np.unique(input).max() + 1
    if order == 0 or not is_label or num_classes < 3:
        if multi_class:
            planes = np.array([_zoom(c, scale, order, mode, cval) for c in to_tensor(input)])
            return to_numpy(planes).astype(dtype)
        return _zoom(input, scale, order, mode, cval).astype(dtype)
    planes = np.array([_zoom(c, scale, order, mode, cval) for c in to_one_hot(input, num_classes, to_tensor=True)])
    return np.argmax(planes, axis=0).astype(dtype)


def resize(input, shape, order=1, mode='reflect', cval=0, is_label=False):
    orig = input.shape
    multi_class = len(shape) == len(orig) - 1
    scale = np.array(shape) / np.array(orig[:len(shape)])
    return rescale(input, scale, order=order, mode=mode, cval=cval, is_label=is_label, multi_class=multi_class)


# ------------------------------------------------------------------ cropping / padding (transform.py:387-437)
def gen_bbox_for_crop(crop_size, orig_shape, crop_margin, crop_mode):
    assert crop_mode == "center" or crop_mode == "random", "crop mode must be either center or random"
    bbox = []
    for i in range(len(orig_shape)):
        if i >= len(crop_size):
            bbox.append([0, orig_shape[i]])
            continue
        room = orig_shape[i] - crop_size[i] - crop_margin[i]
        if crop_mode == 'random' and room > crop_margin[i]:
            lo = np.random.randint(crop_margin[i], room)
        else:
            lo = (orig_shape[i] - crop_size[i]) // 2
        bbox.append([lo, lo + crop_size[i]])
    return bbox


def crop_pad_to_bbox(input, bbox, pad_mode='constant', pad_cval=0):
    shape = input.shape
    inside = tuple(slice(max(0, bbox[d][0]), min(bbox[d][1], shape[d])) for d in range(len(shape)))
    out = input[inside]
    widths = [[abs(min(0, bbox[d][0])), abs(min(0, shape[d] - bbox[d][1]))] for d in range(len(shape))]
    if any(w > 0 for pair in widths for w in pair):
        out = np.pad(out, widths, pad_mode, constant_values=pad_cval)
    return out.astype(input.dtype)


def crop_pad(input, crop_size, crop_mode='center', crop_margin=0, pad_mode='constant', pad_cval=0):
    margin = _per_axis(crop_margin, len(crop_size))
    return crop_pad_to_bbox(input, gen_bbox_for_crop(crop_size, input.shape, margin, crop_mode), pad_mode, pad_cval)


def pad(input, pad_size, pad_mode='constant', pad_cval=0):
    size = [max(input.shape[d], pad_size[d]) for d in range(len(pad_size))]
    return crop_pad(input, size, pad_mode=pad_mode, pad_cval=pad_cval)


# ------------------------------------------------------------------ labels (transform.py:5-20, 323-384)
def label_components(mask):
    """Connected components (6-connectivity) of the non-zero voxels: (labels int32, K), the components numbered in the
    order of their first voxel.  numpy in -> scipy.ndimage.label; HIP tensor in -> the kernels of csrc/components.hip,
    an int32 HIP tensor out, with the same numbering."""
    if torch.is_tensor(mask):
        import components
        return components.label(mask)
    labels, count = ndi.label(mask)
    return labels, int(count)


def remove_small_region(input, threshold):
    """numpy: as the reference.  A HIP tensor is labelled, measured and filtered on the device; like the numpy route it
    is modified in place and returned."""
    if torch.is_tensor(input):
        import components
        return components.remove_small_region(input, threshold)
    labels, _ = ndi.label(input)
    areas = np.bincount(labels.ravel())
    input[(areas < threshold)[labels]] = 0
    return input


# ------------------------------------------------------------------ binary morphology + clean-up (nb_post.py:88-112)
def _binary_morphology(name, input, structure, iterations, border_value):
    """numpy in -> scipy.ndimage.<name>, boolean numpy out; HIP tensor in -> pack (!= 0), the kernels of
    csrc/morphology.hip, unpack: a torch.bool HIP tensor of the input's shape with the same voxels set."""
    if torch.is_tensor(input):
        import components
        import morphology
        fn = {'binary_erosion': morphology.erode, 'binary_dilation': morphology.dilate,
              'binary_opening': morphology.open, 'binary_closing': morphology.close}[name]
        result = fn(morphology.pack(components.as_mask(input)), structure, iterations, border_value)
        return morphology.unpack(result, 1, out=torch.empty(input.shape, dtype=torch.bool, device=input.device))
    return getattr(ndi, name)(input, structure=structure, iterations=iterations, border_value=border_value)


def binary_erosion(input, structure=None, iterations=1, border_value=0):
    """scipy.ndimage.binary_erosion (structure None = the centre and its 6 neighbours) for numpy arrays and HIP tensors."""
    return _binary_morphology('binary_erosion', input, structure, iterations, border_value)


def binary_dilation(input, structure=None, iterations=1, border_value=0):
    """scipy.ndimage.binary_dilation for numpy arrays and HIP tensors."""
    return _binary_morphology('binary_dilation', input, structure, iterations, border_value)


def binary_opening(input, structure=None, iterations=1, border_value=0):
    """scipy.ndimage.binary_opening (erosions, then dilations) for numpy arrays and HIP tensors."""
    return _binary_morphology('binary_opening', input, structure, iterations, border_value)


def binary_closing(input, structure=None, iterations=1, border_value=0):
    """scipy.ndimage.binary_closing (dilations, then erosions) for numpy arrays and HIP tensors.  With border_value 0
    the erosion clears what lies within the structure's reach of the volume's faces - scipy's rule, kept."""
    return _binary_morphology('binary_closing', input, structure, iterations, border_value)


def binary_propagation(input, structure=None, mask=None, border_value=0):
    """scipy.ndimage.binary_propagation: `input` spread through `mask` (None: everywhere) until nothing changes.
    structure: None (the face neighbours) or the full cube.  numpy in -> scipy, boolean numpy out; HIP tensor in -> pack
    (!= 0), the flood of csrc/propagate.hip, unpack: a torch.bool HIP tensor of the input's shape."""
    if torch.is_tensor(input):
        import components
        import morphology
        if mask is not None and (not torch.is_tensor(mask) or tuple(mask.shape) != tuple(input.shape)):
            raise ValueError("binary_propagation: mask must be a HIP tensor of the input's shape %s" % (tuple(input.shape),))
        seed = morphology.pack(components.as_mask(input))
        allowed = morphology.pack(components.as_mask(mask)) if mask is not None else None
        result = morphology.propagate(seed, allowed, structure, border_value)
        return morphology.unpack(result, 1, out=torch.empty(input.shape, dtype=torch.bool, device=input.device))
    return ndi.binary_propagation(input, structure=structure, mask=mask, border_value=border_value)


def binary_fill_holes(input, structure=None):
    """scipy.ndimage.binary_fill_holes: the non-zero voxels plus what the outside of the volume cannot reach through
    their complement.  numpy in -> scipy; HIP tensor in -> the flood of csrc/propagate.hip, a torch.bool HIP tensor out."""
    if torch.is_tensor(input):
        import components
        import morphology
        result = morphology.fill_holes(morphology.pack(components.as_mask(input)), structure)
        return morphology.unpack(result, 1, out=torch.empty(input.shape, dtype=torch.bool, device=input.device))
    return ndi.binary_fill_holes(input, structure=structure)


def _check_k(what, k, limit=8):
    if isinstance(k, bool) or int(k) != k or not 1 <= k <= limit:
        raise ValueError("%s: k=%r (1 .. %d)" % (what, k, limit))
    return int(k)


def keep_largest_region(input, k=1):
    """Zero everything but the `k` largest components (6-connectivity) of the non-zero voxels, 1 <= k <= 8; among equal
    sizes the component met first wins.  Like remove_small_region, `input` is modified in place and returned.  numpy ->
    scipy.ndimage.label; a HIP tensor is labelled, measured, picked and filtered on the device."""
    k = _check_k("keep_largest_region", k)
    if torch.is_tensor(input):
        import components
        return components.keep_largest_region(input, k)
    labels, _ = ndi.label(input)
    sizes = np.bincount(labels.ravel())[1:]
    keep = np.zeros(sizes.size + 1, dtype=bool)
    keep[np.argsort(-sizes, kind='stable')[:k] + 1] = True
    input[~keep[labels]] = 0
    return input


def _label_table(what, table):
    """{label: value} with integer keys (a recipe read back from JSON has them as strings), ascending."""
    out = {}
    for key, value in dict(table or {}).items():
        label = int(key)
        if not 1 <= label <= 255:
            raise ValueError("clean_labels: %s names the label %r (1 .. 255)" % (what, key))
        out[label] = value
    return dict(sorted(out.items()))


def clean_labels(input, foreground=None, keep_largest=None, min_voxels=None, fill_holes=(), structure=None):
    """The clean-up of a predicted label map, a new uint8 volume; `input` is left as it is.
      1. foreground=k: only the k largest components of `input > 0` survive.
      2. for each label, ascending, named in min_voxels ({label: t}) or keep_largest ({label: k}): the components of
         `== label` with fewer than t voxels become 0, then all but the k largest.
      3. for each label of fill_holes, in the given order: the holes of `== label` (binary_fill_holes, `structure`)
         are painted with the label where the volume is 0; another label enclosed in it stays.
    numpy in -> scipy; a uint8 HIP tensor in -> csrc/components.hip and csrc/propagate.hip, a uint8 HIP tensor out with
    the same voxels."""
    keep_largest = {label: _check_k("clean_labels: keep_largest", k) for label, k in
                    _label_table("keep_largest", keep_largest).items()}
    min_voxels = _label_table("min_voxels", min_voxels)
    fill = [int(label) for label in fill_holes]
    if any(not 1 <= label <= 255 for label in fill):
        raise ValueError("clean_labels: fill_holes=%r (labels 1 .. 255)" % (fill_holes,))
    if foreground is not None:
        foreground = _check_k("clean_labels: foreground", foreground)
    device = torch.is_tensor(input)
    if device:
        import morphology
        if input.dtype != torch.uint8:
            raise ValueError("clean_labels: expected a uint8 label volume on the device, got %s" % input.dtype)
        output = input.clone(memory_format=torch.contiguous_format)
    else:
        output = np.array(input, dtype=np.uint8)
    if foreground is not None:
        if device:
            keep_largest_region(output, foreground)                  # non-zero bytes are the mask: dropped ones are zeroed
        else:
            output[~keep_largest_region(output > 0, foreground)] = 0
    for label in sorted(set(min_voxels) | set(keep_largest)):
        if device:
            before = morphology.pack(output, 'eq', label)
            kept = morphology.unpack(before, 1)
        else:
            before = output == label
            kept = before.copy()
        if label in min_voxels:
            remove_small_region(kept, min_voxels[label])
        if label in keep_largest:
            keep_largest_region(kept, keep_largest[label])
        if device:
            morphology.unpack(before, 0, out=output, paint=True)
            morphology.unpack(morphology.pack(kept), label, out=output, paint=True)
        else:
            output[before & ~kept] = 0
    for label in fill:
        if device:
            filled = morphology.fill_holes(morphology.pack(output, 'eq', label), structure)
            filled.bits &= morphology.pack(output, 'eq', 0).bits      # paint only where the volume is 0
            morphology.unpack(filled, label, out=output, paint=True)
        else:
            output[ndi.binary_fill_holes(output == label, structure=structure) & (output == 0)] = label
    return output


def distance_transform_edt(input, sampling=None, squared=False):
    """scipy.ndimage.distance_transform_edt: the Euclidean distance, in `sampling` units, of every non-zero voxel to the
    nearest zero voxel (zero voxels get 0), or its square with `squared=True`.  numpy in -> scipy, float64 numpy out; a
    HIP tensor of 1 to 3 axes -> the exact transform of csrc/distance.hip, float64 HIP tensor out.  The one departure
    from scipy: an input without any zero voxel gives inf everywhere on the device route."""
    if torch.is_tensor(input):
        import components
        import distance
        import morphology
        sq = distance.edt_squared(morphology.pack(components.as_mask(input), 'eq', 0), sampling)
        return sq if squared else sq.sqrt_()
    out = ndi.distance_transform_edt(input, sampling=sampling)
    return out * out if squared else out


# ------------------------------------------------------------------ surface meshes (contract: include/ru3d.h)
# corners q0 .. q3 of the quad of direction d (-x, +x, -y, +y, -z, +z) as offsets from the voxel's own corner: for +u,
# (u, v, w) cyclic, the far-u corners with (v, w) offsets 00 10 11 01; for -u the near-u corners with 00 01 11 10
def _quad_offsets():
    table = np.zeros((6, 4, 3), dtype=np.int64)
    for u in range(3):
        v, w = (u + 1) % 3, (u + 2) % 3
        for far, steps in ((0, ((0, 0), (0, 1), (1, 1), (1, 0))), (1, ((0, 0), (1, 0), (1, 1), (0, 1)))):
            for c, (dv, dw) in enumerate(steps):
                table[2 * u + far, c, u] = far
                table[2 * u + far, c, v] = dv
                table[2 * u + far, c, w] = dw
    return table


_QUAD_OFFSETS = _quad_offsets()


def _mixed(blocks):
    """neither all set nor all unset, over a list of boolean arrays of one shape"""
    some, every = blocks[0].copy(), blocks[0].copy()
    for b in blocks[1:]:
        some |= b
        every &= b
    return some & ~every


def _extract_mesh_numpy(mask):
    """(corners int32 [V, 3], faces int32 [2 Q, 3], neighbours int32 [V, 6]) of a boolean volume [X, Y, Z] from the
    plain definition.  The work is done on the mask's bounding box: corner order and quad order are lexicographic, so
    cropping changes no number."""
    if not mask.any():
        return np.zeros((0, 3), np.int32), np.zeros((0, 3), np.int32), np.zeros((0, 6), np.int32)
    lo = [int(np.flatnonzero(mask.any(axis=tuple(a for a in range(3) if a != ax)))[0]) for ax in range(3)]
    hi = [int(np.flatnonzero(mask.any(axis=tuple(a for a in range(3) if a != ax)))[-1]) + 1 for ax in range(3)]
    m = mask[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
    X, Y, Z = m.shape
    p = np.zeros((X + 2, Y + 2, Z + 2), dtype=bool)                         # voxel (x, y, z) at p[x + 1, y + 1, z + 1]
    p[1:-1, 1:-1, 1:-1] = m
    cshape = (X + 1, Y + 1, Z + 1)

    def around(a, b, c):                                                   # voxels (i - 1 + a, j - 1 + b, k - 1 + c)
        return p[a:a + X + 1, b:b + Y + 1, c:c + Z + 1]

    vertex = _mixed([around(a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)])
    linear = np.flatnonzero(vertex)                                         # sorted: a corner's number is its rank here
    corners = np.stack(np.unravel_index(linear, cshape), axis=1)

    def number(ijk):
        return np.searchsorted(linear, np.ravel_multi_index((ijk[..., 0], ijk[..., 1], ijk[..., 2]), cshape))

    inner = p[1:-1, 1:-1, 1:-1]
    beside = (p[:-2, 1:-1, 1:-1], p[2:, 1:-1, 1:-1], p[1:-1, :-2, 1:-1], p[1:-1, 2:, 1:-1], p[1:-1, 1:-1, :-2],
              p[1:-1, 1:-1, 2:])
    quads = np.argwhere(np.stack([inner & ~b for b in beside], axis=-1))    # [Q, 4]: x, y, z, d
    q = number(quads[:, None, :3] + _QUAD_OFFSETS[quads[:, 3]])            # [Q, 4]
    faces = np.stack((q[:, [0, 1, 2]], q[:, [0, 2, 3]]), axis=1).reshape(-1, 3)

    # the lattice edge leaving corner (i, j, k) in direction -u / +u is surrounded by the voxels with u = i_u - 1 / i_u
    neighbours = np.full((len(corners), 6), -1, dtype=np.int64)
    at = (corners[:, 0], corners[:, 1], corners[:, 2])
    for u in range(3):
        for far in (0, 1):
            pick = [(0, 1)] * 3
            pick[u] = (far,)
            edge = _mixed([around(a, b, c) for a in pick[0] for b in pick[1] for c in pick[2]])[at]
            step = corners[edge].copy()
            step[:, u] += 2 * far - 1
            neighbours[edge, 2 * u + far] = number(step)
    corners = corners + np.array(lo)
    return corners.astype(np.int32), faces.astype(np.int32), neighbours.astype(np.int32)


def _umbrella_numpy(p, neighbours, factor):
    """One umbrella step of the contract: s = 0 plus the present neighbours in direction order, q = p + f (s / m - p)."""
    present = neighbours >= 0
    s = np.zeros_like(p)
    for d in range(6):
        s = s + np.where(present[:, d:d + 1], p[np.maximum(neighbours[:, d], 0)], 0.0)
    m = present.sum(axis=1, keepdims=True).astype(np.float64)
    moved = p + np.float64(factor) * (s / np.maximum(m, 1.0) - p)
    return np.where(m > 0, moved, p)


def _measure_mesh_numpy(vertices, faces):
    """(area, enclosed volume) of a triangle list: half the sum of |(p1 - p0) x (p2 - p0)|, a sixth of the sum of
    p0 . (p1 x p2)."""
    if not len(faces):
        return 0.0, 0.0
    a, b, c = (vertices[faces[:, k]] for k in range(3))
    area = 0.5 * np.sqrt((np.cross(b - a, c - a) ** 2).sum(axis=1)).sum()
    return float(area), float((a * np.cross(b, c)).sum() / 6.0)


def _to_world_numpy(vertices, faces, affine):
    """The numpy twin of mesh.to_world: same expression, same order."""
    import mesh
    r, t, flipped = mesh.world_terms(affine)
    out = vertices[:, 0:1] * r[:, 0] + vertices[:, 1:2] * r[:, 1] + vertices[:, 2:3] * r[:, 2] + t
    return out, (np.ascontiguousarray(faces[:, [0, 2, 1]]) if flipped else faces)


def extract_mesh(input, smooth_iterations=10, lam=0.5, mu=-0.53):
    """The closed triangle mesh around the non-zero voxels of a volume of 1 to 3 axes, Taubin-smoothed on the lattice's
    edge graph: a `mesh.Mesh` with `corners`, `vertices` (float64, voxel coordinates: voxel centres on integers),
    `faces` (counter-clockwise seen from outside), `neighbours` and `shape`.  numpy in -> the definition of
    include/ru3d.h in vectorised numpy, numpy arrays out; HIP tensor in -> the kernels of csrc/mesh.hip, HIP tensors
    out, the same numbers either way.  Unsmoothed (`smooth_iterations=0`) the mesh is the voxels' own faces: its volume
    is the voxel count and its area the number of exposed faces."""
    import mesh
    if int(smooth_iterations) != smooth_iterations or smooth_iterations < 0:
        raise ValueError("extract_mesh: smooth_iterations=%r (a count >= 0)" % (smooth_iterations,))
    if torch.is_tensor(input):
        import components
        import morphology
        if input.dim() < 1 or input.dim() > 3:
            raise ValueError("extract_mesh: expected a volume of 1 to 3 axes, got shape %s" % (tuple(input.shape),))
        return mesh.smooth(mesh.extract(morphology.pack(components.as_mask(input))), smooth_iterations, lam, mu)
    volume = np.asarray(input) != 0
    if volume.ndim < 1 or volume.ndim > 3:
        raise ValueError("extract_mesh: expected a volume of 1 to 3 axes, got shape %s" % (volume.shape,))
    corners, faces, neighbours = _extract_mesh_numpy(volume.reshape((1,) * (3 - volume.ndim) + volume.shape))
    vertices = corners.astype(np.float64) - 0.5
    for _ in range(int(smooth_iterations)):
        vertices = _umbrella_numpy(_umbrella_numpy(vertices, neighbours, lam), neighbours, mu)
    return mesh.Mesh(corners, vertices, faces, neighbours, volume.shape)


# ------------------------------------------------------------------ curve skeletons (contract: include/ru3d.h)
# The 3 x 3 x 3 neighbourhood of a voxel as a 27-bit code: bit 9 (dx + 1) + 3 (dy + 1) + (dz + 1), the voxel itself bit 13.
_SK_ALL, _SK_N26, _SK_N18, _SK_N6 = 0x7ffffff, 0x7ffdfff, 0x2ebdeba, 0x415410
# cells a step along +z, -z, +y, -y may land on (the cells whose z is not 0, not 2, whose y is not 0, not 2)
_SK_NZ0, _SK_NZ2, _SK_NY0, _SK_NY2 = 0x6db6db6, 0x36db6db, 0x7e3f1f8, 0xfc7e3f
_SK_DIRECTIONS = ((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1))
# the 13 offsets that name every unordered pair of 26-adjacent voxels once: cells 14 .. 26 of the code, in that order
_SK_HALF = tuple((i // 9 - 1, (i // 3) % 3 - 1, i % 3 - 1) for i in range(14, 27))


def _sk_grow26(r):
    """The cells of a code and everything 26-adjacent to them inside the cube: three 1-D dilations, one per axis."""
    r = r | ((r << 1) & _SK_NZ0) | ((r >> 1) & _SK_NZ2)
    r = r | ((r << 3) & _SK_NY0) | ((r >> 3) & _SK_NY2)
    return (r | (r << 9) | (r >> 9)) & _SK_ALL


def _sk_grow6(r):
    """The cells of a code and their face neighbours inside the cube."""
    return (r | ((r << 1) & _SK_NZ0) | ((r >> 1) & _SK_NZ2) | ((r << 3) & _SK_NY0) | ((r >> 3) & _SK_NY2)
            | (r << 9) | (r >> 9)) & _SK_ALL


def _sk_fill(seed, allowed, grow):
    """Flood fill of `seed` inside `allowed` (uint32 arrays of codes) until nothing grows any more."""
    reach = seed
    while True:
        grown = grow(reach) & allowed
        if np.array_equal(grown, reach):
            return reach
        reach = grown


def _sk_simple(code):
    """Simple voxels (T26 = 1 and T6bar = 1) among the object voxels whose neighbourhood codes are `code` (uint32)."""
    code = np.asarray(code, dtype=np.uint32)
    obj = code & np.uint32(_SK_N26)
    seed = obj ^ (obj & (obj - np.uint32(1)))                              # the lowest set bit (0 stays 0)
    t26 = (obj != 0) & (_sk_fill(seed, obj, _sk_grow26) == obj)
    back = ~code & np.uint32(_SK_N18)
    faces = back & np.uint32(_SK_N6)
    seed = faces ^ (faces & (faces - np.uint32(1)))
    t6 = (faces != 0) & ((faces & ~_sk_fill(seed, back, _sk_grow6)) == 0)
    return t26 & t6


def _sk_end(code):
    """End voxels: exactly one object voxel among the 26 neighbours."""
    return np.bitwise_count(np.asarray(code, dtype=np.uint32) & np.uint32(_SK_N26)) == 1


def _sk_codes(padded, x, y, z):
    """Neighbourhood codes of the voxels (x, y, z) of the volume whose zero-padded copy (one voxel a side) is `padded`."""
    code = np.zeros(len(x), dtype=np.uint32)
    for i in range(27):
        code |= padded[x + i // 9, y + (i // 3) % 3, z + i % 3].astype(np.uint32) << np.uint32(i)
    return code


def _skeleton_numpy(volume, max_iterations=None):
    """(curve skeleton, iterations run) of a boolean volume [X, Y, Z]: the thinning include/ru3d.h defines, in vectorised
    numpy.  The iteration that deletes nothing and ends the run is counted."""
    X, Y, Z = volume.shape
    padded = np.zeros((X + 2, Y + 2, Z + 2), dtype=bool)
    core = padded[1:-1, 1:-1, 1:-1]
    core[...] = volume
    iterations = 0
    while max_iterations is None or iterations < max_iterations:
        deleted = 0
        for dx, dy, dz in _SK_DIRECTIONS:
            cx, cy, cz = np.nonzero(core & ~padded[1 + dx:X + 1 + dx, 1 + dy:Y + 1 + dy, 1 + dz:Z + 1 + dz])
            subfield = 4 * (cx & 1) + 2 * (cy & 1) + (cz & 1)
            for s in range(8):
                pick = subfield == s
                if not pick.any():
                    continue
                x, y, z = cx[pick], cy[pick], cz[pick]
                code = _sk_codes(padded, x, y, z)
                kill = _sk_simple(code) & ~_sk_end(code)
                core[x[kill], y[kill], z[kill]] = False
                deleted += int(kill.sum())
        iterations += 1
        if not deleted:
            break
    return core.copy(), iterations


def _skeleton_neighbours_numpy(skel):
    """int [X, Y, Z]: the number of set voxels among the 26 neighbours of every voxel."""
    X, Y, Z = skel.shape
    padded = np.zeros((X + 2, Y + 2, Z + 2), dtype=np.int32)
    padded[1:-1, 1:-1, 1:-1] = skel
    count = -padded[1:-1, 1:-1, 1:-1]
    for i in range(27):
        count = count + padded[i // 9:X + i // 9, (i // 3) % 3:Y + (i // 3) % 3, i % 3:Z + i % 3]
    return count


def _skeleton_classify_numpy(skel):
    """skeleton.classify on the host: (ends, junctions, n_voxels, n_ends, n_junctions) of a boolean volume [X, Y, Z]."""
    count = _skeleton_neighbours_numpy(skel)
    ends, junctions = skel & (count == 1), skel & (count >= 3)
    return ends, junctions, int(skel.sum()), int(ends.sum()), int(junctions.sum())


def _skeleton_step_lengths(spacing):
    """The 13 step lengths of _SK_HALF in `spacing` units: sqrt(fl(A + fl(B + C))), A = fl(fl(sx dx)^2), in float64."""
    sx, sy, sz = (float(s) for s in spacing)
    return [math.sqrt((sx * dx) * (sx * dx) + ((sy * dy) * (sy * dy) + (sz * dz) * (sz * dz))) for dx, dy, dz in _SK_HALF]


def _skeleton_length_numpy(skel, spacing):
    """skeleton.length on the host: the pairs of 26-adjacent set voxels counted per offset of _SK_HALF, then
    total = fl(total + fl(count * step)) in that order."""
    X, Y, Z = skel.shape
    padded = np.zeros((X + 2, Y + 2, Z + 2), dtype=bool)
    padded[1:-1, 1:-1, 1:-1] = skel
    total = 0.0
    for (dx, dy, dz), step in zip(_SK_HALF, _skeleton_step_lengths(spacing)):
        pairs = int((skel & padded[1 + dx:X + 1 + dx, 1 + dy:Y + 1 + dy, 1 + dz:Z + 1 + dz]).sum())
        total = total + float(pairs) * step
    return total


def _skeleton_components_numpy(kind, lin):
    """(labels int64 [X, Y, Z], count, first voxel of each) of the 26-connected components of a boolean volume, numbered
    in the order of their first voxel (linear index `lin`)."""
    lab, count = ndi.label(kind, np.ones((3, 3, 3), dtype=bool))
    lab = lab.astype(np.int64)
    if not count:
        return lab, 0, np.zeros(0, dtype=np.int64)
    first = np.atleast_1d(ndi.minimum(lin, lab, np.arange(1, count + 1))).astype(np.int64)
    order = np.argsort(first, kind='stable')
    remap = np.zeros(count + 1, dtype=np.int64)
    remap[order + 1] = np.arange(1, count + 1)
    return remap[lab], count, first[order]


def _skeleton_graph_numpy(skel, sq=None, spacing=(1, 1, 1)):
    """skeleton.graph on the host, and the definition the device is held to (include/ru3d.h, "skeleton graph"): a
    boolean volume [X, Y, Z] as nodes (the 26-connected components of the voxels that do not have exactly two set
    neighbours) and branches (those of the voxels that do).  The same dict as skeleton.graph with `ids` a numpy int32
    vector.  sq: the squared radii, as a float64 volume of skel's shape or as the vector over skel's voxels in element
    order; with it the dict has radius_min, radius_mean, radius_max per branch."""
    skel = np.asarray(skel, dtype=bool)
    X, Y, Z = skel.shape
    path = skel & (_skeleton_neighbours_numpy(skel) == 2)
    node = skel & ~path
    lin = np.arange(X * Y * Z, dtype=np.int64).reshape(X, Y, Z)
    node_label, M, node_first = _skeleton_components_numpy(node, lin)
    branch_label, B, _ = _skeleton_components_numpy(path, lin)
    signed = branch_label - node_label                                      # +b on a path voxel, -m on a node voxel
    node_table = np.zeros((M, 6), dtype=np.int64)
    branch_table = np.zeros((B, 18), dtype=np.int64)
    m = node_label[node] - 1
    node_table[:, 0] = np.bincount(m, minlength=M)
    for column, coordinate in zip((2, 3, 4), np.nonzero(node)):
        np.add.at(node_table[:, column], m, coordinate)
    node_table[:, 5] = node_first
    branch_table[:, 0] = np.bincount(branch_label[path] - 1, minlength=B)
    branch_table[:, 1:5] = -1
    padded = np.zeros((X + 2, Y + 2, Z + 2), dtype=np.int64)
    padded[1:-1, 1:-1, 1:-1] = signed
    attachments = [np.zeros((0, 3), dtype=np.int64)]
    for cell in range(27):
        if cell == 13:
            continue
        dx, dy, dz = cell // 9 - 1, (cell // 3) % 3 - 1, cell % 3 - 1
        other = padded[1 + dx:X + 1 + dx, 1 + dy:Y + 1 + dy, 1 + dz:Z + 1 + dz]
        touch = (signed > 0) & (other < 0)                                  # a path voxel p and the node voxel p + o
        np.add.at(node_table[:, 1], -other[touch] - 1, 1)
        attachments.append(np.stack((signed[touch], lin[touch], -other[touch]), axis=1))
        if cell > 13:                                                       # every unordered pair once
            edge = (signed != 0) & (other != 0) & ((signed > 0) | (other > 0))
            np.add.at(branch_table[:, 5 + cell - 14], np.where(signed > 0, signed, other)[edge] - 1, 1)
    attachments = np.concatenate(attachments)
    attachments = attachments[np.lexsort((attachments[:, 2], attachments[:, 1], attachments[:, 0]))]
    per_branch = np.bincount(attachments[:, 0] - 1, minlength=B)
    assert ((per_branch == 0) | (per_branch == 2)).all()                    # a simple path or a closed loop
    open_ = per_branch == 2
    branch_table[open_, 1], branch_table[open_, 2] = attachments[0::2, 1], attachments[1::2, 1]
    branch_table[open_, 3], branch_table[open_, 4] = attachments[0::2, 2], attachments[1::2, 2]
    out = {'ids': signed[skel].astype(np.int32), 'n': int(skel.sum()), 'nodes': M, 'branches': B,
           'node_table': node_table, 'branch_table': branch_table}

    sx, sy, sz = (float(s) for s in spacing)
    length = np.zeros(B, dtype=np.float64)
    for k, step in enumerate(_skeleton_step_lengths(spacing)):
        length = length + branch_table[:, 5 + k].astype(np.float64) * step
    x0, y0, z0 = np.unravel_index(np.where(open_, branch_table[:, 1], 0), (X, Y, Z))
    x1, y1, z1 = np.unravel_index(np.where(open_, branch_table[:, 2], 0), (X, Y, Z))
    ax, ay, az = sx * (x1 - x0).astype(np.float64), sy * (y1 - y0).astype(np.float64), sz * (z1 - z0).astype(np.float64)
    chord = np.where(open_, np.sqrt(ax * ax + (ay * ay + az * az)), np.nan)
    with np.errstate(divide='ignore', invalid='ignore'):
        out.update(length=length, chord=chord, tortuosity=np.where(chord > 0, length / chord, np.nan))
    if sq is not None:
        sq = np.asarray(sq, dtype=np.float64)
        values = sq[path] if sq.shape == skel.shape else sq[path[skel]]
        b = branch_label[path] - 1
        rmin_sq, rmax_sq, rsum_q = np.full(B, np.inf), np.zeros(B), np.zeros(B, dtype=np.int64)
        np.minimum.at(rmin_sq, b, values)
        np.maximum.at(rmax_sq, b, values)
        finite = np.isfinite(values)
        np.add.at(rsum_q, b[finite], np.rint(np.sqrt(values[finite]) * float(1 << 24)).astype(np.int64))
        with np.errstate(divide='ignore', invalid='ignore'):
            mean = rsum_q.astype(np.float64) / float(1 << 24) / branch_table[:, 0].astype(np.float64)
        out.update(radius_min=np.sqrt(rmin_sq), radius_mean=np.where(np.isinf(rmax_sq), np.inf, mean),
                   radius_max=np.sqrt(rmax_sq))
    return out


def _skeleton_prune_numpy(skel, min_length, spacing=(1, 1, 1), max_rounds=None):
    """skeleton.prune on the host: (pruned boolean volume, rounds).  A spur is a branch shorter than min_length with
    exactly one end on a node of valence 1 made of a single voxel and the other end on a node of valence >= 3; a round
    erases the path voxels and the end voxel of every spur of the graph as it is when the round begins.  Rounds repeat
    until one finds no spur (that round is counted) or max_rounds."""
    out = np.array(skel, dtype=bool)
    rounds = 0
    while max_rounds is None or rounds < max_rounds:
        g = _skeleton_graph_numpy(out, None, spacing)
        rounds += 1
        nodes, gone = g['node_table'], []
        for b, row in enumerate(g['branch_table']):
            n0, n1 = int(row[3]), int(row[4])
            if n0 < 1 or not g['length'][b] < min_length:
                continue
            for tip, far in ((n0, n1), (n1, n0)):
                if nodes[tip - 1, 0] == 1 and nodes[tip - 1, 1] == 1 and nodes[far - 1, 1] >= 3:
                    gone += [b + 1, -tip]
        if not gone:
            break
        signed = np.zeros(out.shape, dtype=np.int64)
        signed[out] = g['ids']
        out &= ~np.isin(signed, gone)
    return out, rounds


def skeletonize(input, max_iterations=None):
    """The curve skeleton of the non-zero voxels of a bool / uint8 volume of 1 to 3 axes: a topology-preserving thinning
    (objects 26-connected, background 6-connected, outside the volume is background) that deletes simple voxels
    direction by direction and subfield by subfield and keeps end voxels - the contract of include/ru3d.h, "skeleton".
    The result has the input's kind and dtype, the skeleton voxels 1 / True.  numpy in -> the vectorised numpy twin; a
    HIP tensor in -> the kernels of csrc/skeleton.hip, voxel for voxel the same.  max_iterations stops the thinning
    early; `input` is left as it is."""
    if max_iterations is not None and (int(max_iterations) != max_iterations or max_iterations < 0):
        raise ValueError("skeletonize: max_iterations=%r (None or a count >= 0)" % (max_iterations,))
    if torch.is_tensor(input):
        import morphology
        import skeleton
        if input.dtype not in (torch.bool, torch.uint8):
            raise ValueError("skeletonize: expected a bool or uint8 volume, got %s" % input.dtype)
        thin = skeleton.thin(morphology.pack(input), max_iterations)
        return morphology.unpack(thin, 1, out=torch.empty(input.shape, dtype=input.dtype, device=input.device))
    volume = np.asarray(input)
    if volume.dtype not in (np.bool_, np.uint8):
        raise ValueError("skeletonize: expected a bool or uint8 volume, got %s" % volume.dtype)
    if volume.ndim < 1 or volume.ndim > 3:
        raise ValueError("skeletonize: expected a volume of 1 to 3 axes, got shape %s" % (volume.shape,))
    skel, _ = _skeleton_numpy((volume != 0).reshape((1,) * (3 - volume.ndim) + volume.shape), max_iterations)
    return skel.reshape(volume.shape).astype(volume.dtype)


def create_sphere(shape, center, r):
    """nb_post.py:81-85: integer array of `shape`, 1 where the distance to `center` is at most r."""
    x, y, z = np.ogrid[:shape[0], :shape[1], :shape[2]]
    return 1 * (np.sqrt((x - center[0]) ** 2 + (y - center[1]) ** 2 + (z - center[2]) ** 2) <= r)


def post_transform(input, threshold=10000, label=2, structure=None):
    """The clean-up of a predicted label volume (nb_post.py:88-112): 1 on the components of `input > 0` that have at
    least `threshold` voxels, and `label` where `input == label` survives a closing by `structure` (None: the 251-voxel
    ball create_sphere((7, 7, 7), (3, 3, 3), 4)) and an opening by the 6-neighbour cross.  numpy in -> scipy; a uint8
    HIP tensor in -> packed masks on the device (morphology.py), a uint8 HIP tensor out.  `input` is left as it is."""
    if structure is None:
        structure = create_sphere((7, 7, 7), (3, 3, 3), 4)
    if torch.is_tensor(input):
        import components
        import morphology
        if input.dtype != torch.uint8:
            raise ValueError("post_transform: expected a uint8 label volume on the device, got %s" % input.dtype)
        output = morphology.unpack(morphology.pack(input, 'gt', 0), 1)
        components.remove_small_region(output, threshold)
        kept = morphology.open(morphology.close(morphology.pack(input, 'eq', label), structure))
        return morphology.unpack(kept, label, out=output, paint=True)
    output = np.zeros_like(input)
    output[remove_small_region(input > 0, threshold)] = 1
    output[ndi.binary_opening(ndi.binary_closing(input == label, structure))] = label
    return output


def combination_labels(input, combinations, num_classes):
    """transform.py:323-363: merge label classes.  `combinations` is one group or a list of groups of class indices.
    The new class order follows the old classes 0, 1, ...: a class that belongs to a group puts that whole group at
    its place (once), a class in no group stays a class of its own; voxels get the index of their (merged) class."""
    groups = [list(combinations)] if np.ndim(combinations[0]) == 0 else [list(g) for g in combinations]
    order, placed = [], set()
    for c in range(num_classes):
        owners = [i for i, g in enumerate(groups) if c in g]
        if not owners:
            order.append([c])
        for i in owners:
            if i not in placed:
                order.append(groups[i])
                placed.add(i)
    onehot = to_one_hot(input, num_classes, to_tensor=True)
    planes = np.array([np.any([onehot[c].astype(bool) for c in group], axis=0) for group in order])
    return np.argmax(planes, axis=0).astype(input.dtype)


# ------------------------------------------------------------------ overlapping label groups (numpy twins of csrc/groups.hip)
def labels_to_groups(label, groups, num_labels=None):
    """Integer label map [...] -> uint8 [K, ...]: plane k is 1 where the voxel's label is a member of groups[k] (the
    multi-hot targets the group losses read through loss.group_table without ever building them).  A label outside
    [0, num_labels) is a member of no group."""
    import loss
    table = np.frombuffer(loss.group_table(groups, num_labels), dtype=np.uint8)
    label = np.asarray(label).astype(np.int64)
    inside = (label >= 0) & (label < len(table))
    bits = np.where(inside, table[np.clip(label, 0, len(table) - 1)], 0)
    return np.stack([(bits >> k) & 1 for k in range(len(groups))]).astype(np.uint8)


def default_group_labels(groups):
    """The label value each group decodes to: the smallest member of group k that belongs to no other group nested
    inside it (a proper subset of it) - the value that tells the group from the structures it contains.
    ((1, 2), (2,)) -> (1, 2); ((2,), (1, 2)) -> (2, 1).  ValueError when the nested groups use a group up, as group 0 of
    ((1, 2), (1,), (2,)): pass group_labels then."""
    import loss
    gs, _ = loss._checked_groups(groups)
    sets = [frozenset(g) for g in gs]
    out = []
    for k, s in enumerate(sets):
        own = set(s)
        for other in sets:
            if other < s:
                own -= other
        if not own:
            raise ValueError("default_group_labels: every member of group %d %s lies in a group nested inside it; "
                             "pass group_labels" % (k, gs[k]))
        out.append(min(own))
    return tuple(out)


def _checked_decode(groups, group_labels, threshold):
    """(K label values, K float32 thresholds) of the decoding arguments, or ValueError."""
    import loss
    groups, _ = loss._checked_groups(groups)
    k = len(groups)
    labels = default_group_labels(groups) if group_labels is None else tuple(int(v) for v in group_labels)
    if len(labels) != k or any(not 0 <= v <= 255 for v in labels):
        raise ValueError("group_labels must hold %d label values of 0 .. 255, got %r" % (k, labels))
    thr = np.asarray(threshold, dtype=np.float32)
    thr = np.full(k, thr, dtype=np.float32) if thr.ndim == 0 else thr
    if thr.shape != (k,) or np.isnan(thr).any():
        raise ValueError("threshold must be a number or %d numbers, got %r" % (k, threshold))
    return labels, thr


def groups_to_labels(prob_or_bits, groups, group_labels=None, threshold=0.5):
    """[..., K] probabilities (float) or on/off bits (bool) -> uint8 label map [...] by the decoding rule of
    ru3d_predict_merge_groups: channel k is on iff its probability is > threshold (a number, or one per group; a NaN is
    off), the voxel gets group_labels[k] (default default_group_labels(groups)) of the LAST channel that is on - later
    groups overwrite earlier ones - and 0 when none is."""
    labels, thr = _checked_decode(groups, group_labels, threshold)
    q = np.asarray(prob_or_bits)
    if q.shape[-1] != len(labels):
        raise ValueError("groups_to_labels: last axis has %d channels for %d groups" % (q.shape[-1], len(labels)))
    on = q if q.dtype == np.bool_ else np.asarray(q, dtype=np.float32) > thr
    out = np.zeros(q.shape[:-1], dtype=np.uint8)
    for k, v in enumerate(labels):
        out[on[..., k]] = v
    return out


# ------------------------------------------------------------------ intensity (transform.py:176-193)
def adjust_contrast(input, factor):
    mean = input.mean()
    return ((input - mean) * factor + mean).astype(input.dtype)


def adjust_brightness(input, factor):
    low = input.min()
    return ((input - low) * factor + low).astype(input.dtype)


def adjust_gamma(input, gamma, epsilon=1e-7):
    low, high = input.min(), input.max()
    span = high - low + epsilon
    return (np.power((input - low) / span, gamma) * span + low).astype(input.dtype)


# ------------------------------------------------------------------ noise, blur, low resolution (module degrade)
def _degrade(image, ops):
    """channels-last image [X, Y, Z, C] (or one volume [X, Y, Z]): numpy in -> the numpy twins of module degrade, float32
    numpy out; HIP tensor in -> the kernels of csrc/degrade.hip, a new fp32 HIP tensor out."""
    if torch.is_tensor(image):
        return degrade.apply_device(image, ops)
    image = np.asarray(image)
    if image.ndim == 3:
        return degrade.apply_numpy(image[None], ops)[0]
    return np.ascontiguousarray(to_numpy(degrade.apply_numpy(np.ascontiguousarray(to_tensor(image)), ops)))


def philox4x32(counter, key):
    """Philox4x32-10 of 32-bit counter words [..., 4] under key (k0, k1) -> uint32 [..., 4]."""
    return degrade.philox4x32(counter, key)


def gaussian_noise(image, variance, key):
    """image + sqrt(variance) * n, n standard normals from Philox4x32-10 under key (k0, k1) and Box-Muller in float64:
    the voxel with linear index i over [C][x][y][z] takes normal i & 3 of the call with counter (i >> 2, 0, 0, 0)."""
    return _degrade(image, {"noise": (float(variance), (int(key[0]), int(key[1])))})


def gaussian_blur(image, sigma):
    """scipy.ndimage.gaussian_filter(channel, sigma) with scipy's defaults (mode='reflect', truncate=4) on every channel:
    passes along x, y, z accumulated in float64 and stored as float32.  The radius int(4 sigma + 0.5) may be at most 16
    and at most the smallest extent."""
    return _degrade(image, {"blur": float(sigma)})


def simulate_low_resolution(image, zoom):
    """Every channel nearest-neighbour down to the grid max(round(P * zoom), 2) and order 1 back up to P:
    resize(resize(x, n, order=0), P, order=1), as one gather in float64 rounded to float32 once.  0 < zoom <= 1."""
    return _degrade(image, {"low_res": float(zoom)})


# ------------------------------------------------------------------ transform classes
class _ImageFactor(object):
    """One uniform draw from a range, applied to case['image'] (RandomContrast / Brightness / Gamma: :196-259)."""
    fn = None

    def __init__(self, factor_range):
        self.factor_range = _as_range(factor_range)

    def __call__(self, case):
        factor = np.random.uniform(self.factor_range[0], self.factor_range[1])
        case['image'] = type(self).fn(case['image'], factor)
        return case


class RandomContrast(_ImageFactor):
    fn = staticmethod(adjust_contrast)


class RandomBrightness(_ImageFactor):
    fn = staticmethod(adjust_brightness)


class RandomGamma(_ImageFactor):
    fn = staticmethod(adjust_gamma)

    def __init__(self, gamma_range):
        super().__init__(gamma_range)
        self.gamma_range = self.factor_range


class _RandomDegrade(object):
    """With probability p, one of the three ops of module degrade on case['image'] with a parameter drawn from `range`:
    the draws of DeviceAugment(noise= / blur= / low_res=(p, range)), from numpy's global generator."""
    name = None

    def __init__(self, p, range):
        check = {"noise": degrade.check_noise, "blur": degrade.check_blur, "low_res": degrade.check_low_res}[self.name]
        self.p, self.range = check((p, range))

    def __call__(self, case):
        ops = degrade.draw(np.random, **{k: (self.p, self.range) if k == self.name else None
                                         for k in ("noise", "blur", "low_res")})
        if ops:
            case['image'] = _degrade(case['image'], ops)
        return case


class RandomGaussianNoise(_RandomDegrade):
    name = "noise"


class RandomGaussianBlur(_RandomDegrade):
    name = "blur"


class RandomLowResolution(_RandomDegrade):
    name = "low_res"


class RandomMirror(object):
    def __init__(self, p_per_axis):
        self.p_per_axis = p_per_axis

    def __call__(self, case):
        self.p_per_axis = _per_axis(self.p_per_axis, len(case['image'].shape) - 1)
        for axis, p in enumerate(self.p_per_axis):
            if np.random.uniform() < p:
                case['image'] = np.flip(case['image'], axis).copy()
                case['label'] = np.flip(case['label'], axis).copy()
        return case


class ToTensor(object):
    def __call__(self, case):
        case['image'] = to_tensor(case['image'])
        return case


class ToNumpy(object):
    def __call__(self, case):
        case['image'] = to_numpy(case['image'])
        return case


class ToOnehot(object):
    def __init__(self, num_classes, to_tensor=False):
        self.num_classes, self.to_tensor = num_classes, to_tensor

    def __call__(self, case):
        case['label'] = to_one_hot(case['label'], self.num_classes, self.to_tensor)
        return case


class CombineLabels(object):
    def __init__(self, combinations, num_classes):
        self.combinations, self.num_classes = combinations, num_classes

    def __call__(self, case):
        case['label'] = combination_labels(case['label'], self.combinations, self.num_classes)
        return case


class RemoveSmallRegion(object):
    def __init__(self, threshold):
        self.threshold = threshold

    def __call__(self, case):
        case['label'] = remove_small_region(case['label'], self.threshold)
        return case


class KeepLargestRegion(object):
    """keep_largest_region on case[key] (the label by default, like RemoveSmallRegion)."""

    def __init__(self, k=1, key='label'):
        self.k, self.key = k, key

    def __call__(self, case):
        case[self.key] = keep_largest_region(case[self.key], self.k)
        return case


class CleanLabels(object):
    """clean_labels on case['pred'] with the keywords of a recipe (trainer.determine_postprocessing), for numpy cases
    and cases that live on the device."""

    def __init__(self, **recipe):
        self.recipe = recipe

    def __call__(self, case):
        case['pred'] = clean_labels(case['pred'], **self.recipe)
        return case


class PostTransform(object):
    """post_transform on case[key] (the prediction by default), for numpy cases and cases that live on the device."""

    def __init__(self, threshold=10000, label=2, structure=None, key='pred'):
        self.threshold, self.label, self.structure, self.key = threshold, label, structure, key

    def __call__(self, case):
        case[self.key] = post_transform(case[self.key], self.threshold, self.label, self.structure)
        return case


class Skeletonize(object):
    """skeletonize on case[key] (the prediction by default), for numpy cases and cases that live on the device.
    label=None thins the non-zero voxels; label=k thins `case[key] == k`.  The result replaces case[key] as a uint8
    volume of the same kind with 1 on the skeleton."""

    def __init__(self, key='pred', label=None):
        self.key, self.label = key, label

    def __call__(self, case):
        volume = case[self.key]
        picked = (volume != 0) if self.label is None else (volume == self.label)
        as_bytes = picked.to(torch.uint8) if torch.is_tensor(picked) else np.asarray(picked).astype(np.uint8)
        case[self.key] = skeletonize(as_bytes)
        return case


class Resize(object):
    def __init__(self, shape):
        self.shape = shape

    def __call__(self, case):
        case['image'] = resize(case['image'], self.shape)
        case['label'] = resize(case['label'], self.shape, is_label=True)
        return case


class RandomRescale(object):
    def __init__(self, scale):
        self.scale = _as_range(scale)

    def __call__(self, case):
        s = np.random.uniform(self.scale[0], self.scale[1])
        case['image'] = rescale(case['image'], s)
        case['label'] = rescale(case['label'], s, is_label=True)
        return case


class Crop(object):
    """transform.py:440-511: crop image and label with one box; retry until every enforce_label_indices entry is in
    the cropped label.

    oversample_foreground = p in (0, 1] (not in the reference): with probability p the box is placed on a voxel drawn from
    the label's class-location index instead (module `locations`: rule and draw order; foreground_classes: the values to
    draw from, None = every value >= 1 present).  The index is class_locations(label, max_locations), computed per call
    unless the case carries one under 'class_index'.  The numpy twin of DeviceAugment(oversample_foreground=...)."""

    def __init__(self, crop_size=128, crop_mode='center', crop_margin=0, enforce_label_indices=[],
                 image_pad_mode='constant', image_pad_cval=0, label_pad_mode='constant', label_pad_cval=0,
                 oversample_foreground=None, foreground_classes=None, max_locations=10000):
        self.crop_size, self.crop_mode, self.crop_margin = crop_size, crop_mode, crop_margin
        self.enforce_label_indices = ([enforce_label_indices] if isinstance(enforce_label_indices, int)
                                      else enforce_label_indices)
        self.image_pad_mode, self.image_pad_cval = image_pad_mode, image_pad_cval
        self.label_pad_mode, self.label_pad_cval = label_pad_mode, label_pad_cval
        self.oversample, self.foreground_classes, self.max_locations = locations.check_oversample(
            oversample_foreground, foreground_classes, max_locations, crop_mode, self.enforce_label_indices)

    def _placed(self, label, size, index):
        """The oversampling draws: the box of a forced patch, or None for a box drawn the usual way."""
        def rows():
            counts, _, found = index if index is not None else class_locations(label, self.max_locations)
            return counts, found.__getitem__
        lo = locations.draw_forced_box(np.random, self.oversample, self.foreground_classes, rows, list(size)[:3],
                                       label.shape, self.crop_margin)
        return lo and [[lo[i], lo[i] + int(size[i])] for i in range(3)]

    def _box(self, image, label, size, index=None):
        placed = self._placed(label, size, index) if self.oversample is not None else None
        while True:
            bbox = placed + [[0, image.shape[-1]]] if placed else \
                gen_bbox_for_crop(size, image.shape, self.crop_margin, self.crop_mode)
            cropped = crop_pad_to_bbox(label, bbox[:-1], self.label_pad_mode, self.label_pad_cval)
            present = np.unique(cropped)
            if all(i in present for i in self.enforce_label_indices):
                return bbox, cropped

    def __call__(self, case):
        dim = len(case['image'].shape) - 1
        self.crop_size = _per_axis(self.crop_size, dim)
        self.crop_margin = _per_axis(self.crop_margin, dim)
        bbox, cropped_label = self._box(case['image'], case['label'], self.crop_size, case.get('class_index'))
        case['image'] = crop_pad_to_bbox(case['image'], bbox, self.image_pad_mode, self.image_pad_cval)
        case['label'] = cropped_label
        return case


class RandomCrop(Crop):
    def __init__(self, crop_size=128, crop_margin=0, enforce_label_indices=[], image_pad_mode='constant',
                 image_pad_cval=0, label_pad_mode='constant', label_pad_cval=0, oversample_foreground=None,
                 foreground_classes=None, max_locations=10000):
        super().__init__(crop_size, crop_mode='random', crop_margin=crop_margin,
                         enforce_label_indices=enforce_label_indices, image_pad_mode=image_pad_mode,
                         image_pad_cval=image_pad_cval, label_pad_mode=label_pad_mode, label_pad_cval=label_pad_cval,
                         oversample_foreground=oversample_foreground, foreground_classes=foreground_classes,
                         max_locations=max_locations)


class CenterCrop(Crop):
    def __init__(self, crop_size=128, image_pad_mode='constant', image_pad_cval=0, label_pad_mode='constant',
                 label_pad_cval=0):
        super().__init__(crop_size, crop_mode='center', image_pad_mode=image_pad_mode, image_pad_cval=image_pad_cval,
                         label_pad_mode=label_pad_mode, label_pad_cval=label_pad_cval)


class RandomRescaleCrop(Crop):
    """transform.py:573-652: draw a scale, crop round(size / scale), resize the crop to `size`."""

    def __init__(self, scale, crop_size=128, crop_mode='center', crop_margin=0, enforce_label_indices=[],
                 image_pad_mode='constant', image_pad_cval=0, label_pad_mode='constant', label_pad_cval=0,
                 oversample_foreground=None, foreground_classes=None, max_locations=10000):
        super().__init__(crop_size, crop_mode=crop_mode, crop_margin=crop_margin,
                         enforce_label_indices=enforce_label_indices, image_pad_mode=image_pad_mode,
                         image_pad_cval=image_pad_cval, label_pad_mode=label_pad_mode, label_pad_cval=label_pad_cval,
                         oversample_foreground=oversample_foreground, foreground_classes=foreground_classes,
                         max_locations=max_locations)
        self.scale = _as_range(scale)

    def __call__(self, case):
        dim = len(case['image'].shape) - 1
        self.crop_size = _per_axis(self.crop_size, dim)
        self.crop_margin = _per_axis(self.crop_margin, dim)
        s = np.random.uniform(self.scale[0], self.scale[1])
        before = np.round(np.array(self.crop_size) / s).astype(int)       # the reference's np.int (gone in numpy 1.24)
        bbox, cropped_label = self._box(case['image'], case['label'], before, case.get('class_index'))
        cropped_image = crop_pad_to_bbox(case['image'], bbox, self.image_pad_mode, self.image_pad_cval)
        case['image'] = resize(cropped_image, self.crop_size)
        case['label'] = resize(cropped_label, self.crop_size, is_label=True)
        return case


class RandomSpatialCrop(Crop):
    """RandomRescaleCrop with a rotation about the crop box's centre and a cubic B-spline elastic deformation (module
    spatial: geometry and draw order): the numpy twin of DeviceAugment(rotation=..., elastic_spacing=...,
    elastic_magnitude=...).  Scale and crop box are drawn as RandomRescaleCrop draws them, enforce_label_indices and the
    label rule's class count look at that axis-aligned box; the patch is cut *around* it (a rotated or deformed patch
    reaches outside it, and outside the volume it reads the pad constants).  With zero angles and a zero lattice the
    patch is RandomRescaleCrop's."""

    def __init__(self, scale, crop_size=128, rotation=None, elastic_spacing=None, elastic_magnitude=None,
                 crop_mode='center', crop_margin=0, enforce_label_indices=[], image_pad_cval=0, label_pad_cval=0,
                 label_margin=False, oversample_foreground=None, foreground_classes=None, max_locations=10000):
        super().__init__(crop_size, crop_mode=crop_mode, crop_margin=crop_margin,
                         enforce_label_indices=enforce_label_indices, image_pad_cval=image_pad_cval,
                         label_pad_cval=label_pad_cval, oversample_foreground=oversample_foreground,
                         foreground_classes=foreground_classes, max_locations=max_locations)
        self.scale = _as_range(scale)
        self.rotation = spatial.check_rotation(rotation)
        self.elastic = spatial.check_elastic(elastic_spacing, elastic_magnitude)
        self.label_margin = label_margin       # also store case['label_margin'] (resample_at's return_margin)

    def __call__(self, case):
        self.crop_size = _per_axis(self.crop_size, 3)
        self.crop_margin = _per_axis(self.crop_margin, 3)
        s = np.random.uniform(self.scale[0], self.scale[1])
        before = np.round(np.array(self.crop_size) / s).astype(int)
        bbox, cropped_label = self._box(case['image'], case['label'], before, case.get('class_index'))
        angles, phi = spatial.draw_spatial(np.random, self.rotation, self.elastic, self.crop_size)
        centre, matrix = spatial.patch_geometry([b[0] for b in bbox[:3]], before, self.crop_size, angles)
        coords = spatial_coordinates(self.crop_size, centre, matrix, phi, self.elastic and self.elastic[0])
        case['image'] = resample_at(case['image'], coords, self.image_pad_cval).astype(case['image'].dtype)
        label = resample_at(case['label'], coords, self.label_pad_cval, is_label=True,
                            num_classes=int(np.unique(cropped_label).max()) + 1, return_margin=self.label_margin)
        if self.label_margin:
            label, case['label_margin'] = label
        case['label'] = label
        return case


# ------------------------------------------------------------------ nearest site / territories (contract: include/ru3d.h)
def _nearest_pass_numpy(value, step, axis):
    """One pass of the separable feature transform along `axis` of a float64 volume: (least fl(fl(fl(step (l - l'))^2) +
    value[l']) over l', the smallest l' that attains it).  argmin takes the first of equal candidates."""
    v = np.moveaxis(value, axis, -1)
    L = v.shape[-1]
    rows = v.reshape(-1, L)
    t = step * (np.arange(L)[:, None] - np.arange(L)[None, :]).astype(np.float64)
    sq = t * t                                                              # [l, l']
    best = np.empty(rows.shape, dtype=np.float64)
    arg = np.empty(rows.shape, dtype=np.int64)
    chunk = max(1, (1 << 22) // (L * L))
    for r in range(0, len(rows), chunk):
        cand = sq[None, :, :] + rows[r:r + chunk, None, :]
        a = cand.argmin(axis=-1)
        arg[r:r + chunk] = a
        best[r:r + chunk] = np.take_along_axis(cand, a[..., None], axis=-1)[..., 0]
    return np.moveaxis(best.reshape(v.shape), -1, axis), np.moveaxis(arg.reshape(v.shape), -1, axis)


def _nearest_site_numpy(sites, spacing=(1, 1, 1)):
    """The definition ru3d_nearest_site is held to (include/ru3d.h, "nearest site / territories"): (index int32, sq
    float64) of a bool volume [X, Y, Z] of sites - the linear index of the nearest site of every voxel, chosen pass by
    pass (z, then y, then x) by value with the smaller coordinate winning a tie, and the squared distance
    fl(A + fl(B + C)) to it.  No site: -1 and inf."""
    sites = np.asarray(sites, dtype=bool)
    X, Y, Z = sites.shape
    sx, sy, sz = (float(s) for s in spacing)
    value, at_z = _nearest_pass_numpy(np.where(sites, 0.0, np.inf), sz, 2)
    value, at_y = _nearest_pass_numpy(value, sy, 1)
    site = at_y * Z + np.take_along_axis(at_z, at_y, axis=1)
    value, at_x = _nearest_pass_numpy(value, sx, 0)
    site = at_x * (Y * Z) + np.take_along_axis(site, at_x, axis=0)
    return np.where(np.isinf(value), -1, site).astype(np.int32), value


def _site_assign_numpy(sites, site_ids, index, region=None):
    """ru3d_site_assign on the host: int32 labels, site_ids[rank of index[p] among the sites in element order] where
    `region` (None: everywhere) is set and index[p] >= 0, 0 elsewhere."""
    sites = np.asarray(sites, dtype=bool)
    site_ids = np.asarray(site_ids, dtype=np.int32)
    if site_ids.shape != (int(sites.sum()),):
        raise ValueError("site_assign: %s ids for %d sites" % (site_ids.shape, int(sites.sum())))
    rank = np.cumsum(sites.reshape(-1)) - 1
    take = index >= 0 if region is None else (index >= 0) & np.asarray(region, dtype=bool)
    if not sites.reshape(-1)[index[take]].all():
        raise ValueError("site_assign: an index that is not a site")
    labels = np.zeros(sites.shape, dtype=np.int32)
    labels[take] = site_ids[rank[index[take]]]
    return labels


def _territory_tally_numpy(labels, K, other=None, num_other=0, region=None):
    """ru3d_territory_tally on the host: int64 [K + 1, num_other + 1], the voxels of `region` (None: all) per label and
    per min(other, num_other)."""
    cols = int(num_other) + 1
    if other is None and num_other:
        raise ValueError("territory_tally: num_other=%r without `other`" % (num_other,))
    take = np.ones(labels.shape, dtype=bool) if region is None else np.asarray(region, dtype=bool)
    l = labels[take].astype(np.int64)
    if l.size and (l.min() < 0 or l.max() > K):
        raise ValueError("territory_tally: a label outside 0 .. %d" % K)
    o = np.minimum(other[take].astype(np.int64), num_other) if other is not None else 0
    return np.bincount(l * cols + o, minlength=(int(K) + 1) * cols).astype(np.int64).reshape(int(K) + 1, cols)


def nearest_feature(input, sampling=None):
    """(index, squared distance) of the nearest non-zero voxel of `input` (1 to 3 axes) for every voxel: index is int32,
    the linear index into the volume (-1 without any non-zero voxel), the squared distance float64 in `sampling` units
    (inf then).  Among equally near voxels the choice is the one of include/ru3d.h, "nearest site / territories".
    numpy in -> the numpy twin, numpy out; a HIP tensor in -> the kernels of csrc/territory.hip, HIP tensors out, equal
    to the twin element for element."""
    import distance
    if torch.is_tensor(input):
        import components
        import morphology
        import territory
        return territory.nearest(morphology.pack(components.as_mask(input)), sampling)
    volume = np.asarray(input)
    if volume.ndim < 1 or volume.ndim > 3:
        raise ValueError("nearest_feature: expected a volume of 1 to 3 axes, got shape %s" % (volume.shape,))
    spacing = distance._spacing(sampling, volume.ndim)
    index, sq = _nearest_site_numpy((volume != 0).reshape((1,) * (3 - volume.ndim) + volume.shape), spacing)
    return index.reshape(volume.shape), sq.reshape(volume.shape)


# ------------------------------------------------------------------ geodesic distance (contract: include/ru3d.h)
def _geodesic_numpy(seeds, allowed, weights, limit):
    """The definition ru3d_geodesic_rounds is held to (include/ru3d.h, "geodesic distance"): (dist uint32, labels int32) of
    an integer volume [X, Y, Z] of seeds (0: none, > 0: a label) grown through the bool volume `allowed` (None:
    everywhere) - a heap Dijkstra on (dist, label) over the steps of geodesic.OFFSETS with the integer lengths `weights`
    (0: no such step), a step taken only when it ends at a distance <= limit.  Not reached: 0xFFFFFFFF and 0.  With the
    limit that stands for none (0xFFFFFFFE) an allowed voxel left unreached beside a reached one raises OverflowError."""
    import heapq
    from geodesic import OFFSETS, UNLIMITED, UNREACHED
    seeds = np.asarray(seeds)
    if seeds.ndim != 3:
        raise ValueError("geodesic: a volume of shape %s (three axes here)" % (seeds.shape,))
    if (seeds < 0).any():
        raise ValueError("geodesic: a negative value among the seeds (0: no seed, > 0: a label)")
    X, Y, Z = seeds.shape
    open_ = np.zeros((X + 2, Y + 2, Z + 2), dtype=bool)                      # a closed rim instead of bounds checks
    open_[1:-1, 1:-1, 1:-1] = True if allowed is None else np.asarray(allowed, dtype=bool)
    sy, sx = Z + 2, (Y + 2) * (Z + 2)
    # weight k is the step INTO a voxel from its neighbour at offset k, so it leads from p to p - offset
    steps = [(-(dx * sx + dy * sy + dz), int(w)) for (dx, dy, dz), w in zip(OFFSETS, weights) if int(w)]
    is_open = open_.reshape(-1).tolist()
    dist, label = [UNREACHED] * open_.size, [0] * open_.size
    heap = []
    for x, y, z in np.argwhere(seeds > 0):
        p = (x + 1) * sx + (y + 1) * sy + z + 1
        dist[p], label[p] = 0, int(seeds[x, y, z])
        heap.append((0, label[p], p))
    heapq.heapify(heap)
    limit = int(limit)
    while heap:
        d, l, p = heapq.heappop(heap)
        if d != dist[p] or l != label[p]:
            continue
        for o, w in steps:
            q = p + o
            if is_open[q] and d + w <= limit and (d + w < dist[q] or (d + w == dist[q] and l < label[q])):
                dist[q], label[q] = d + w, l
                heapq.heappush(heap, (d + w, l, q))
    dist = np.array(dist, dtype=np.int64).reshape(open_.shape)
    label = np.array(label, dtype=np.int64).reshape(open_.shape)
    if limit == UNLIMITED:
        reached, stuck = dist != UNREACHED, open_ & (dist == UNREACHED)
        for (dx, dy, dz), w in zip(OFFSETS, weights):
            if int(w) and (stuck & np.roll(reached, (-dx, -dy, -dz), axis=(0, 1, 2))).any():  # the rim is never reached
                raise OverflowError("geodesic: a distance beyond %d quanta - choose a larger quantum, or a max_distance"
                                    % UNLIMITED)
    return dist[1:-1, 1:-1, 1:-1].astype(np.uint32), label[1:-1, 1:-1, 1:-1].astype(np.int32)


def geodesic_distance(seeds, mask=None, sampling=None, structure=None, quantum=2.0 ** -10, max_distance=None):
    """(distance, labels): for every voxel the length of the shortest path to a seed that stays inside `mask` (None:
    everywhere) and the label of that seed.  seeds: an integer volume of 1 to 3 axes, 0 = no seed, > 0 = the seed's
    label; a seed outside the mask stays and spreads into its neighbours inside.  The path runs over the face steps
    (structure None) or all 26 (the full cube) and every step counts its Euclidean length under `sampling`, rounded to a
    multiple of `quantum`, so the sums are integers and the answer is unique: the smallest distance and, among equally
    near seeds, the smallest label (include/ru3d.h, "geodesic distance").  distance is float64 in sampling units, inf
    where no path arrives (or none within max_distance); labels int32, 0 there.  numpy in -> the numpy twin, numpy out;
    HIP tensors in -> csrc/geodesic.hip, HIP tensors out, equal to the twin element for element."""
    import geodesic
    if torch.is_tensor(seeds):
        import components
        import morphology
        if mask is not None and (not torch.is_tensor(mask) or tuple(mask.shape) != tuple(seeds.shape)):
            raise ValueError("geodesic_distance: mask must be a HIP tensor of the seeds' shape %s" % (tuple(seeds.shape),))
        if seeds.dtype in (torch.uint8, torch.bool, torch.int8, torch.int16, torch.int64):
            seeds = seeds.to(torch.int32)
        allowed = morphology.pack(components.as_mask(mask)) if mask is not None else None
        dist, labels = geodesic.grow(seeds, allowed, sampling, structure, quantum, max_distance)
        return geodesic.millimetres(dist, quantum), labels
    volume = np.asarray(seeds)
    if volume.ndim < 1 or volume.ndim > 3:
        raise ValueError("geodesic_distance: expected a volume of 1 to 3 axes, got shape %s" % (volume.shape,))
    if mask is not None and np.shape(mask) != volume.shape:
        raise ValueError("geodesic_distance: mask of shape %s for seeds of shape %s" % (np.shape(mask), volume.shape))
    import morphology
    weights = geodesic.step_weights(sampling, volume.ndim, morphology._connectivity(structure, volume.ndim, "geodesic_distance"),
                                    quantum)
    shape3 = (1,) * (3 - volume.ndim) + volume.shape
    dist, labels = _geodesic_numpy(volume.reshape(shape3), None if mask is None else (np.asarray(mask) != 0).reshape(shape3),
                                   weights, geodesic.distance_limit(max_distance, quantum))
    out = dist.astype(np.float64) * float(quantum)
    out[dist == geodesic.UNREACHED] = np.inf
    return out.reshape(volume.shape), labels.reshape(volume.shape)


# ------------------------------------------------------------------ local thickness (contract: include/ru3d.h)
def _contract_d2_numpy(a, b, spacing):
    """d2 of include/ru3d.h between two lists of voxels, int64 [n, 3] and [m, 3]: float64 [n, m], fl(A + fl(B + C)) with
    A = fl(fl(sx (ax - bx))^2), B and C alike."""
    sq = [(float(spacing[k]) * (a[:, None, k] - b[None, :, k]).astype(np.float64)) ** 2 for k in range(3)]
    return sq[0] + (sq[1] + sq[2])


def _inscribed_squared_numpy(mask3, spacing=(1, 1, 1)):
    """R2 of include/ru3d.h, "local thickness", of a bool volume [X, Y, Z]: float64, for every voxel of the mask the
    least d2 to a clear voxel inside the volume by brute force over all pairs, 0 on the clear voxels, +inf everywhere
    when there is none."""
    mask3 = np.asarray(mask3, dtype=bool)
    r2 = np.zeros(mask3.shape, dtype=np.float64)
    inside, clear = np.argwhere(mask3).astype(np.int64), np.argwhere(~mask3).astype(np.int64)
    if not len(clear):
        r2[...] = np.inf
        return r2
    chunk = max(1, (1 << 21) // len(clear))
    best = np.empty(len(inside), dtype=np.float64)
    for i in range(0, len(inside), chunk):
        best[i:i + chunk] = _contract_d2_numpy(inside[i:i + chunk], clear, spacing).min(axis=1)
    r2[mask3] = best
    return r2


def _local_thickness_numpy(mask3, spacing=(1, 1, 1)):
    """The definition ru3d_thickness_paint is held to (include/ru3d.h, "local thickness"): T2 (float64) of a bool volume
    [X, Y, Z], T2(x) = max { R2(p) : p in M, d2(x, p) < R2(p) } on the mask M and 0 off it, a direct evaluation over
    all pairs of mask voxels with R2 by the same expression (_inscribed_squared_numpy).  No clear voxel: +inf on every
    voxel.  Quadratic in the mask's voxels: a yardstick for small volumes, not a tool."""
    mask3 = np.asarray(mask3, dtype=bool)
    if mask3.ndim != 3:
        raise ValueError("local_thickness: a volume of shape %s (three axes here)" % (mask3.shape,))
    r2 = _inscribed_squared_numpy(mask3, spacing)
    if mask3.all():
        return r2                                                           # +inf everywhere (or an empty volume)
    t2 = np.zeros(mask3.shape, dtype=np.float64)
    inside = np.argwhere(mask3).astype(np.int64)
    if not len(inside):
        return t2
    radius = r2[mask3]                                                      # [p], element order
    chunk = max(1, (1 << 21) // len(inside))
    best = np.empty(len(inside), dtype=np.float64)
    for i in range(0, len(inside), chunk):
        covered = _contract_d2_numpy(inside[i:i + chunk], inside, spacing) < radius[None, :]
        best[i:i + chunk] = np.where(covered, radius[None, :], 0.0).max(axis=1)
    t2[mask3] = best
    return t2


def local_thickness(input, sampling=None, squared=False):
    """The local thickness of the non-zero voxels of `input` (1 to 3 axes): for every voxel the diameter 2 sqrt(T2), in
    `sampling` units, of the largest ball that fits inside the structure and contains the voxel (include/ru3d.h, "local
    thickness"); 0 outside the structure, inf everywhere when the structure fills the volume (the volume's faces are not
    background).  squared=True returns T2 itself, the squared radius.  Distances run between voxel centres: a slab of k
    voxels reads k voxels thick for even k and k + 1 for odd k.  numpy in -> the numpy twin (quadratic in the
    structure's voxels), numpy out; a HIP tensor in -> csrc/thickness.hip, a float64 HIP tensor out, T2 equal to the
    twin element for element."""
    import distance
    if torch.is_tensor(input):
        import components
        import morphology
        import thickness
        t2 = thickness.local_squared(morphology.pack(components.as_mask(input)), sampling)
        return t2 if squared else thickness.diameter(t2)
    volume = np.asarray(input)
    if volume.ndim < 1 or volume.ndim > 3:
        raise ValueError("local_thickness: expected a volume of 1 to 3 axes, got shape %s" % (volume.shape,))
    spacing = distance._spacing(sampling, volume.ndim)
    t2 = _local_thickness_numpy((volume != 0).reshape((1,) * (3 - volume.ndim) + volume.shape), spacing).reshape(volume.shape)
    return t2 if squared else 2.0 * np.sqrt(t2)
