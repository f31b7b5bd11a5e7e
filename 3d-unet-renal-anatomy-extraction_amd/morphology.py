"""Binary morphology on bit-packed masks and the confusion table of two label volumes on the device
(csrc/morphology.hip).

The host code these replace when the volumes live in HBM: `scipy.ndimage.binary_erosion / _dilation / _opening /
_closing` of the reference's clean-up (nb_post.py:88-112) and the per-class float reductions of its evaluation
(trainer.py:348-356, nb.py:11-37).  A mask is held as a `PackedMask`: 64 voxels of the contiguous Z axis per 64-bit
word, so `pred == 2` is formed straight from the uint8 prediction and a 512x512x256 mask is 8 MB.  The results are
scipy's, voxel for voxel, including its border rule (voxels outside the volume read as `border_value`) and the
reflection of the structure in a dilation.  `propagate` and `fill_holes` (csrc/propagate.hip) are
`scipy.ndimage.binary_propagation` and `binary_fill_holes` on the same masks: a flood by rounds that never builds a
label volume.  There is no host fallback in here: every function wants HIP tensors.
"""
import functools

import numpy as np
import torch

import _native as N
from _native import check, ptr, stream
from components import MAX_VOXELS, _volume3

_OPS = {'ne': N.MASK_NE, 'eq': N.MASK_EQ, 'gt': N.MASK_GT, 'ge': N.MASK_GE}
_REACH = N.MORPH_MAX_EXTENT // 2


class PackedMask:
    """`bits`: int64 HIP tensor [X, Y, ceil(Z / 64)], bit b of word w of row (x, y) = voxel z = 64 w + b (the bits at
    z >= Z are 0); `shape`: the shape of the volume it was packed from (1 to 3 axes)."""

    def __init__(self, bits, shape):
        self.bits = bits
        self.shape = tuple(int(s) for s in shape)
        self.shape3 = (1,) * (3 - len(self.shape)) + self.shape

    @property
    def device(self):
        return self.bits.device

    def new(self):
        return PackedMask(torch.empty_like(self.bits), self.shape)


def _bytes3(volume, what):
    """uint8 view [X, Y, Z] of a contiguous uint8 / bool HIP tensor of 1 to 3 axes."""
    if not torch.is_tensor(volume):
        raise ValueError("%s: expected a HIP tensor, got %s" % (what, type(volume).__name__))
    if volume.dtype not in (torch.uint8, torch.bool):
        raise ValueError("%s: expected a uint8 or bool volume, got %s" % (what, volume.dtype))
    if volume.numel() == 0 or volume.numel() >= MAX_VOXELS:
        raise ValueError("%s: a volume of %d voxels is not supported (1 .. 2**31 - 1)" % (what, volume.numel()))
    if volume.dim() < 1 or volume.dim() > 3:
        raise ValueError("%s: expected a volume of 1 to 3 axes, got shape %s" % (what, tuple(volume.shape)))
    N.require_device(volume, what)
    volume = volume.contiguous()
    return _volume3(volume.view(torch.uint8) if volume.dtype == torch.bool else volume, what)


def pack(volume, op='ne', value=0):
    """Bits of `volume != 0` ('ne'), `== value` ('eq'), `> value` ('gt') or `>= value` ('ge') of a uint8 / bool HIP
    tensor of 1 to 3 axes."""
    if op not in _OPS:
        raise ValueError("pack: op must be one of 'ne', 'eq', 'gt', 'ge', got %r" % (op,))
    if not 0 <= int(value) <= 255:
        raise ValueError("pack: value %r is not a uint8" % (value,))
    shape = tuple(volume.shape) if torch.is_tensor(volume) else ()
    v = _bytes3(volume, "pack: volume")
    X, Y, Z = (int(s) for s in v.shape)
    bits = torch.empty((X, Y, (Z + 63) // 64), dtype=torch.int64, device=v.device)
    check(N.lib.ru3d_mask_pack(ptr(v), X, Y, Z, _OPS[op], int(value), ptr(bits), stream()), "mask_pack")
    return PackedMask(bits, shape)


def unpack(mask, value=1, out=None, paint=False):
    """uint8 HIP tensor of the mask's shape: `value` where the bit is set and 0 elsewhere, or with `paint=True`
    `out[mask] = value` on an existing volume (`out` is required then, and returned)."""
    if not 0 <= int(value) <= 255:
        raise ValueError("unpack: value %r is not a uint8" % (value,))
    if out is None:
        if paint:
            raise ValueError("unpack: paint=True needs the volume to paint into (out=)")
        out = torch.empty(mask.shape, dtype=torch.uint8, device=mask.device)
    elif (not torch.is_tensor(out) or out.dtype not in (torch.uint8, torch.bool) or not out.is_contiguous()
          or tuple(out.shape) != mask.shape or out.device != mask.device):
        raise ValueError("unpack: out must be a contiguous uint8 or bool tensor of shape %s on %s" % (mask.shape, mask.device))
    X, Y, Z = mask.shape3
    N.note_device(mask.device)
    dst = out.view(torch.uint8) if out.dtype == torch.bool else out
    check(N.lib.ru3d_mask_unpack(ptr(mask.bits), X, Y, Z, int(value), 1 if paint else 0, ptr(dst), stream()), "mask_unpack")
    return out


# ------------------------------------------------------------------------------------------------ structuring elements
def default_structure():
    """scipy.ndimage.generate_binary_structure(3, 1): the centre and its six neighbours."""
    s = np.zeros((3, 3, 3), dtype=bool)
    s[1, 1, :] = s[1, :, 1] = s[:, 1, 1] = True
    return s


def _structure3(structure, ndim):
    """Boolean numpy structure [sx, sy, sz] for a volume of `ndim` axes, checked against what the kernel does."""
    if structure is None:
        structure = default_structure()[(1,) * (3 - ndim)]
    if torch.is_tensor(structure):
        structure = structure.cpu().numpy()
    s = np.asarray(structure) != 0
    if s.ndim != ndim:
        raise ValueError("structure: %d axes for a volume of %d axes" % (s.ndim, ndim))
    s = s.reshape((1,) * (3 - s.ndim) + s.shape)
    for extent in s.shape:
        if extent % 2 == 0:
            raise ValueError("structure: even extent in shape %s (odd extents with the origin at the centre only)"
                             % (s.shape,))
        if extent > N.MORPH_MAX_EXTENT:
            raise ValueError("structure: extent above %d in shape %s" % (N.MORPH_MAX_EXTENT, s.shape))
    if not s.any():
        raise ValueError("structure: no element is set")
    return s


def structure_rows(structure, reflect=False):
    """The table the kernel walks: one (dx, dy, zmask) per (x, y) row of a 3-axis structure that has an element set,
    bit k of zmask standing for the z offset k - 7.  Offsets are relative to the centre; `reflect` negates them (a
    dilation gathers in[p - s])."""
    s = _structure3(structure, 3)
    cx, cy, cz = (e // 2 for e in s.shape)
    sign = -1 if reflect else 1
    zmasks = (s * (1 << (sign * (np.arange(s.shape[2]) - cz) + _REACH))).sum(axis=2)
    return sorted((sign * (int(ix) - cx), sign * (int(iy) - cy), int(zmasks[ix, iy])) for ix, iy in np.argwhere(zmasks))


def _check_args(what, iterations, border_value, origin, mask):
    if int(iterations) != iterations or iterations < 1:
        raise ValueError("%s: iterations=%r (a positive count; 'until nothing changes' is not supported)"
                         % (what, iterations))
    if border_value not in (0, 1, False, True):
        raise ValueError("%s: border_value=%r (0 or 1)" % (what, border_value))
    if np.any(np.asarray(origin) != 0):
        raise ValueError("%s: origin=%r (only the centred origin 0 is supported)" % (what, origin))
    if mask is not None:
        raise ValueError("%s: a mask= argument is not supported" % what)


@functools.lru_cache(maxsize=64)
def _table(shape, data, reflect):
    """The ctypes row table of a checked 3-axis boolean structure (its shape and bytes), kept per structure: the ball of
    post_transform is built once."""
    rows = structure_rows(np.frombuffer(data, dtype=bool).reshape(shape), reflect)
    return (N.MorphRow * len(rows))(*[N.MorphRow(dx, dy, zm) for dx, dy, zm in rows])


def _morph(src, dst, op, table, border_value):
    X, Y, Z = src.shape3
    N.note_device(src.device)
    check(N.lib.ru3d_binary_morph(ptr(src.bits), ptr(dst.bits), X, Y, Z, op, table, len(table), int(border_value),
                                  stream()), "binary_morph")


def _run(mask, steps, structure, border_value):
    """steps: [(op, count), ...] applied in order, ping-ponging between two packed buffers; `mask` is left as it is."""
    if not isinstance(mask, PackedMask):
        raise ValueError("expected a PackedMask (morphology.pack), got %s" % type(mask).__name__)
    s = _structure3(structure, len(mask.shape))
    key = (s.shape, np.ascontiguousarray(s).tobytes())
    tables = {N.MORPH_ERODE: _table(*key, False), N.MORPH_DILATE: _table(*key, True)}
    src, spare = mask, None
    for op, count in steps:
        for _ in range(int(count)):
            dst = spare if spare is not None else mask.new()
            _morph(src, dst, op, tables[op], border_value)
            spare = src if src is not mask else None
            src = dst
    return src


def erode(input, structure=None, iterations=1, border_value=0, origin=0, mask=None):
    """scipy.ndimage.binary_erosion of a PackedMask: out[p] = AND over s in S of in[p + s]."""
    _check_args("erode", iterations, border_value, origin, mask)
    return _run(input, [(N.MORPH_ERODE, iterations)], structure, border_value)


def dilate(input, structure=None, iterations=1, border_value=0, origin=0, mask=None):
    """scipy.ndimage.binary_dilation of a PackedMask: out[p] = OR over s in S of in[p - s]."""
    _check_args("dilate", iterations, border_value, origin, mask)
    return _run(input, [(N.MORPH_DILATE, iterations)], structure, border_value)


def open(input, structure=None, iterations=1, border_value=0, origin=0, mask=None):
    """scipy.ndimage.binary_opening: `iterations` erosions, then as many dilations."""
    _check_args("open", iterations, border_value, origin, mask)
    return _run(input, [(N.MORPH_ERODE, iterations), (N.MORPH_DILATE, iterations)], structure, border_value)


def close(input, structure=None, iterations=1, border_value=0, origin=0, mask=None):
    """scipy.ndimage.binary_closing: `iterations` dilations, then as many erosions.  With border_value 0 the erosion
    clears every voxel within the structure's reach of the volume's faces, as scipy's does."""
    _check_args("close", iterations, border_value, origin, mask)
    return _run(input, [(N.MORPH_DILATE, iterations), (N.MORPH_ERODE, iterations)], structure, border_value)


# ------------------------------------------------------------------------------------------------ confusion table
def confusion(pred, label, num_classes):
    """int64 HIP tensor [C + 1, C + 1], C = num_classes <= 32: entry [l][p] counts the voxels with label == l and
    pred == p; every value >= C falls into the last row / column.  pred, label: uint8 HIP tensors of one shape (views
    of any alignment are fine as long as they are contiguous)."""
    C = int(num_classes)
    if not 1 <= C <= N.CONFUSION_MAX_CLASSES:
        raise ValueError("confusion: num_classes=%r (1 .. %d)" % (num_classes, N.CONFUSION_MAX_CLASSES))
    for name, t in (("pred", pred), ("label", label)):
        if not torch.is_tensor(t) or t.dtype != torch.uint8:
            raise ValueError("confusion: %s must be a uint8 HIP tensor" % name)
    if tuple(pred.shape) != tuple(label.shape):
        raise ValueError("confusion: pred has shape %s, label %s" % (tuple(pred.shape), tuple(label.shape)))
    if pred.numel() >= MAX_VOXELS:
        raise ValueError("confusion: pred has %d voxels (below 2**31)" % pred.numel())
    N.require_device(pred, "confusion: pred")
    N.require_device(label, "confusion: label")
    pred, label = pred.contiguous(), label.contiguous()
    table = torch.empty((C + 1, C + 1), dtype=torch.int64, device=pred.device)
    N.note_device(pred.device)
    check(N.lib.ru3d_confusion_counts(ptr(pred), ptr(label), pred.numel(), C, ptr(table), stream()), "confusion_counts")
    return table


# ------------------------------------------------------------------------------------------------ propagation, hole filling
# rounds of the last flood (propagate / fill_holes) of this process, the overshoot of the last batch included
last_rounds = 0


def _connectivity(structure, ndim, what):
    """1 for the centre and its 2 * ndim face neighbours (None), 3 for the full 3 ** ndim cube; nothing else."""
    if structure is None:
        return 1
    if torch.is_tensor(structure):
        structure = structure.cpu().numpy()
    s = np.asarray(structure) != 0
    if s.shape == (3,) * ndim:
        if s.all():
            return 3
        if np.array_equal(s, default_structure()[(1,) * (3 - ndim)]):
            return 1
    raise ValueError("%s: structure must be None (the face neighbours) or the full 3 x 3 x 3 cube, in the form of the "
                     "mask's %d axes" % (what, ndim))


def _flood(allowed, invert, reach, connectivity, border_value):
    """Grow reach.bits to the fixpoint: batches of 8, 16, 32, 64, 64, .. rounds, one download of the batch's counters of
    changed tiles after each; a batch whose last round changed nothing has converged."""
    global last_rounds
    N.require_device(allowed.bits, "the packed mask")
    X, Y, Z = allowed.shape3
    ndim = len(allowed.shape)
    border_axes = (7 & ~((1 << (3 - ndim)) - 1)) if border_value else 0       # only the axes the mask really has
    changed = torch.empty(N.PROPAGATE_MAX_ROUNDS, dtype=torch.int32, device=allowed.device)
    N.note_device(allowed.device)
    rounds, total = 8, 0
    while True:
        check(N.lib.ru3d_binary_propagate(ptr(allowed.bits), 1 if invert else 0, ptr(reach.bits), X, Y, Z, connectivity,
                                          border_axes, rounds, ptr(changed), stream()), "binary_propagate")
        total += rounds
        if int(changed[:rounds].cpu()[-1]) == 0:
            break
        rounds = min(2 * rounds, N.PROPAGATE_MAX_ROUNDS)
    last_rounds = total
    return reach


def _packed(mask, what):
    if not isinstance(mask, PackedMask):
        raise ValueError("%s: expected a PackedMask (morphology.pack), got %s" % (what, type(mask).__name__))
    return mask


def propagate(seed, allowed, structure=None, border_value=0):
    """scipy.ndimage.binary_propagation(seed, structure, mask=allowed, border_value=border_value) of PackedMasks: the
    seed and every voxel of `allowed` that a chain of allowed neighbours connects to it (and, with border_value 1, to
    the outside of the volume).  As in scipy, a seed voxel outside `allowed` stays set and spreads into its allowed
    neighbours.  seed=None is the empty seed, allowed=None the whole volume (one of the two is needed for the shape).
    structure: None (face neighbours) or the full cube.  A new PackedMask; the operands are left as they are."""
    if seed is None and allowed is None:
        raise ValueError("propagate: neither a seed nor an allowed mask")
    like = _packed(allowed, "propagate: allowed") if allowed is not None else _packed(seed, "propagate: seed")
    if border_value not in (0, 1, False, True):
        raise ValueError("propagate: border_value=%r (0 or 1)" % (border_value,))
    connectivity = _connectivity(structure, len(like.shape), "propagate")
    if seed is None:
        reach = PackedMask(torch.zeros_like(like.bits), like.shape)
    else:
        _packed(seed, "propagate: seed")
        if seed.shape != like.shape or seed.device != like.device:
            raise ValueError("propagate: seed of shape %s on %s, allowed of shape %s on %s"
                             % (seed.shape, seed.device, like.shape, like.device))
        reach = PackedMask(seed.bits.clone(), seed.shape)
    if allowed is None:                                     # everywhere: the complement of an empty mask, formed on load
        return _flood(PackedMask(torch.zeros_like(like.bits), like.shape), True, reach, connectivity, border_value)
    return _flood(allowed, False, reach, connectivity, border_value)


def fill_holes(mask, structure=None):
    """scipy.ndimage.binary_fill_holes of a PackedMask: the mask plus every voxel of its complement that the outside of
    the volume does not reach through the complement (structure: the neighbourhood of that flood, None or the cube).
    The complement is formed on load, so the flood needs one packed volume beside the result."""
    _packed(mask, "fill_holes: mask")
    connectivity = _connectivity(structure, len(mask.shape), "fill_holes")
    reach = _flood(mask, True, PackedMask(torch.zeros_like(mask.bits), mask.shape), connectivity, 1)
    out = mask.new()
    X, Y, Z = mask.shape3
    check(N.lib.ru3d_mask_fill_result(ptr(mask.bits), ptr(reach.bits), ptr(out.bits), X, Y, Z, stream()), "mask_fill_result")
    return out
