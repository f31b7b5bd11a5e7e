"""Connected components and the cascade's merge on the device (csrc/components.hip).

The host code these replace when the volumes live in HBM: `scipy.ndimage.label` + `np.bincount` + `ndi.find_objects`
in `remove_small_region` / `regions_crop_case` (reference transform.py:5-11, data.py:464-492) and the float64
`total` / `hits` arithmetic of `cascade_predict_case` (reference trainer.py:203-240).  The labelling reproduces scipy's
numbering element for element (components in the order of their first voxel, 6-connectivity), so everything built on it
returns what the host route returns.  There is no host fallback in here: every function wants HIP tensors.
"""
import math

import numpy as np
import torch

import _native as N
from _native import check, ptr, stream

MAX_VOXELS = 2 ** 31


def _volume3(t, what):
    """[..., X, Y, Z] with at most three axes -> the same memory as [X, Y, Z] (leading axes of length 1)."""
    if t.dim() < 1 or t.dim() > 3:
        raise ValueError("%s: expected a volume of 1 to 3 axes, got shape %s" % (what, tuple(t.shape)))
    return t.reshape((1,) * (3 - t.dim()) + tuple(t.shape))


def as_mask(t):
    """uint8 [X, Y, Z] device mask of the non-zero elements of `t` (no copy when `t` already is one)."""
    N.require_device(t, "mask")
    if t.dtype == torch.bool:
        t = t.contiguous().view(torch.uint8)
    elif t.dtype != torch.uint8:
        t = (t != 0).view(torch.uint8)
    return t.contiguous()


def label(mask):
    """mask: HIP tensor, any dtype, non-zero = foreground.  Returns (labels int32 of the mask's shape, K)."""
    shape = tuple(mask.shape)
    m = _volume3(as_mask(mask), "label_components")
    X, Y, Z = (int(s) for s in m.shape)
    if X * Y * Z == 0:
        return torch.zeros(shape, dtype=torch.int32, device=mask.device), 0
    labels = torch.empty((X, Y, Z), dtype=torch.int32, device=m.device)
    count = torch.zeros(1, dtype=torch.int32, device=m.device)
    nbytes = N.lib.ru3d_components_workspace_bytes(X, Y, Z)
    ws = N.workspace(nbytes, m.device)
    N.note_device(m.device)
    check(N.lib.ru3d_label_components(ptr(m), X, Y, Z, ptr(labels), ptr(count), ptr(ws), ws.numel(), stream()),
          "label_components")
    return labels.reshape(shape), int(count.item())


def stats(labels, count):
    """labels: int32 HIP tensor from `label`, count: its K.  Returns (sizes int32 [K], boxes int32 [K, 6]) on the
    device; a box is (x0, x1, y0, y1, z0, z1) with the upper bounds exclusive, like ndi.find_objects' slices."""
    lab = _volume3(labels, "component_stats")
    X, Y, Z = (int(s) for s in lab.shape)
    sizes = torch.empty(count, dtype=torch.int32, device=lab.device)
    boxes = torch.empty((count, 6), dtype=torch.int32, device=lab.device)
    if count:
        N.note_device(lab.device)
        check(N.lib.ru3d_component_stats(ptr(lab), X, Y, Z, int(count), ptr(sizes), ptr(boxes), stream()),
              "component_stats")
    return sizes, boxes


def filter_small(labels, count, sizes, threshold, mask=None, relabel=False):
    """Zero `mask` (uint8 HIP tensor, in place) where the component has fewer than `threshold` voxels; with `relabel`
    also return the label volume of the survivors, renumbered in order.  Returns (labels or None, kept)."""
    lab = _volume3(labels, "filter_components")
    X, Y, Z = (int(s) for s in lab.shape)
    thr = int(min(max(math.ceil(threshold), -1), MAX_VOXELS - 1))        # size < t  <=>  size < ceil(t) for integer sizes
    out = torch.empty_like(lab) if relabel else None
    kept = torch.zeros(1, dtype=torch.int32, device=lab.device)
    if mask is None and out is None:
        raise ValueError("filter_small: nothing to write (no mask, relabel=False)")
    if mask is not None and (mask.dtype != torch.uint8 or not mask.is_contiguous() or mask.numel() != lab.numel()):
        raise ValueError("filter_small: the mask must be a contiguous uint8 tensor of the labels' shape")
    nbytes = N.lib.ru3d_filter_components_workspace_bytes(int(count))
    ws = N.workspace(nbytes, lab.device)
    N.note_device(lab.device)
    check(N.lib.ru3d_filter_components(ptr(lab), X, Y, Z, int(count), ptr(sizes) if count else None, thr, ptr(mask),
                                       ptr(out), ptr(kept), ptr(ws), ws.numel(), stream()), "filter_components")
    return (out.reshape(labels.shape) if out is not None else None), int(kept.item())


def keep_largest(labels, count, sizes, k=1, mask=None, relabel=False):
    """Zero `mask` (uint8 HIP tensor, in place) outside the `k` largest components (1 <= k <= 8; among equal sizes the
    smaller number wins, `np.argsort(-sizes, kind='stable')[:k]`); with `relabel` also return the label volume of the
    survivors, renumbered in their old order.  The choice is made on the device.  Returns (labels or None, kept)."""
    lab = _volume3(labels, "keep_largest")
    X, Y, Z = (int(s) for s in lab.shape)
    if int(k) != k or not 1 <= k <= N.KEEP_LARGEST_MAX:
        raise ValueError("keep_largest: k=%r (1 .. %d)" % (k, N.KEEP_LARGEST_MAX))
    if mask is None and not relabel:
        raise ValueError("keep_largest: nothing to write (no mask, relabel=False)")
    if mask is not None and (mask.dtype != torch.uint8 or not mask.is_contiguous() or mask.numel() != lab.numel()):
        raise ValueError("keep_largest: the mask must be a contiguous uint8 tensor of the labels' shape")
    if count and (sizes is None or sizes.dtype != torch.int32 or sizes.numel() != int(count)):
        raise ValueError("keep_largest: sizes must be the int32 tensor of %d sizes that `stats` returns" % int(count))
    out = torch.empty_like(lab) if relabel else None
    kept = torch.zeros(1, dtype=torch.int32, device=lab.device)
    nbytes = N.lib.ru3d_filter_components_workspace_bytes(int(count))    # the same layout
    ws = N.workspace(nbytes, lab.device)
    N.note_device(lab.device)
    check(N.lib.ru3d_keep_largest_components(ptr(lab), X, Y, Z, int(count), ptr(sizes) if count else None, int(k),
                                             ptr(mask), ptr(out), ptr(kept), ptr(ws), ws.numel(), stream()),
          "keep_largest_components")
    return (out.reshape(labels.shape) if out is not None else None), int(kept.item())


def _in_place(input, edit):
    """Run edit(labels, count, sizes, mask) on the uint8 mask of `input` and zero `input` where the mask was cleared."""
    labels, count = label(input)
    if count == 0:
        return input
    sizes, _ = stats(labels, count)
    direct = input.dtype in (torch.uint8, torch.bool) and input.is_contiguous()
    mask = input.view(torch.uint8) if direct else as_mask(input)
    edit(labels, count, sizes, mask.reshape(labels.shape))
    if not direct:
        input.masked_fill_(mask.reshape(input.shape) == 0, 0)
    return input


def keep_largest_region(input, k=1):
    """transform.keep_largest_region for a HIP tensor: label -> sizes -> pick -> filter, `input` modified in place."""
    if int(k) != k or not 1 <= k <= N.KEEP_LARGEST_MAX:
        raise ValueError("keep_largest_region: k=%r (1 .. %d)" % (k, N.KEEP_LARGEST_MAX))
    return _in_place(input, lambda labels, count, sizes, mask: keep_largest(labels, count, sizes, k, mask=mask))


def remove_small_region(input, threshold):
    """transform.remove_small_region for a HIP tensor: label -> sizes -> filter, `input` modified in place."""
    return _in_place(input, lambda labels, count, sizes, mask: filter_small(labels, count, sizes, threshold, mask=mask))


def region_boxes(mask, threshold):
    """Bounding boxes (numpy int64 [R, 3, 2], upper bounds exclusive) of the components of `mask` that have at least
    `threshold` voxels, in scipy's label order: what `ndi.find_objects(ndi.label(remove_small_region(mask, t))[0])`
    yields.  Only the K sizes and boxes cross to the host."""
    labels, count = label(mask)
    if labels.dim() != 3:
        raise ValueError("region_boxes: expected a [X, Y, Z] mask, got shape %s" % (tuple(mask.shape),))
    if count == 0:
        return np.zeros((0, 3, 2), dtype=np.int64)
    sizes, boxes = stats(labels, count)
    table = torch.cat([sizes[:, None], boxes], dim=1).cpu().numpy().astype(np.int64)
    keep = ~(table[:, 0] < threshold)
    return table[keep, 1:].reshape(-1, 3, 2)


def crop_pad_to_bbox(input, bbox, pad_cval=0):
    """transform.crop_pad_to_bbox (constant padding) for a HIP tensor: a device slice into a padded device buffer."""
    shape = tuple(int(s) for s in input.shape)
    nd = len(shape)
    size = tuple(int(bbox[d][1]) - int(bbox[d][0]) for d in range(nd))
    out = torch.full(size, pad_cval, dtype=input.dtype, device=input.device)
    src = tuple(slice(max(0, int(bbox[d][0])), min(int(bbox[d][1]), shape[d])) for d in range(nd))
    dst = tuple(slice(src[d].start - int(bbox[d][0]), src[d].stop - int(bbox[d][0])) for d in range(nd))
    if all(s.stop > s.start for s in src):
        out[dst] = input[src]
    return out


class CascadeAccumulator:
    """`total` (float64 [X, Y, Z, C]) and `hits` (int32 [X, Y, Z]) of cascade_predict_case, resident in HBM."""

    def __init__(self, shape, num_classes, device):
        self.shape = tuple(int(s) for s in shape)
        self.num_classes = int(num_classes)
        if len(self.shape) != 3 or min(self.shape) < 1 or self.shape[0] * self.shape[1] * self.shape[2] >= MAX_VOXELS:
            raise ValueError("CascadeAccumulator: unsupported volume shape %s" % (self.shape,))
        self.total = torch.zeros(self.shape + (self.num_classes,), dtype=torch.float64, device=device)
        self.hits = torch.zeros(self.shape, dtype=torch.int32, device=device)

    def add(self, prob, origin):
        """prob: float32 HIP tensor [rx, ry, rz, C] of one region whose box starts at `origin` (may be negative)."""
        if prob.dim() != 4 or prob.shape[3] != self.num_classes:
            raise ValueError("CascadeAccumulator.add: expected [x, y, z, %d], got %s" % (self.num_classes, tuple(prob.shape)))
        prob = prob.to(torch.float32).contiguous()
        rx, ry, rz = (int(s) for s in prob.shape[:3])
        X, Y, Z = self.shape
        N.note_device(self.total.device)
        check(N.lib.ru3d_region_accumulate(ptr(prob), rx, ry, rz, self.num_classes, int(origin[0]), int(origin[1]),
                                           int(origin[2]), ptr(self.total), ptr(self.hits), X, Y, Z, stream()),
              "region_accumulate")

    def merge(self):
        """uint8 HIP tensor [X, Y, Z]: the averaged maps rounded (one class) or soft-maxed and arg-maxed."""
        X, Y, Z = self.shape
        out = torch.empty(self.shape, dtype=torch.uint8, device=self.total.device)
        N.note_device(self.total.device)
        check(N.lib.ru3d_cascade_merge(ptr(self.total), ptr(self.hits), X, Y, Z, self.num_classes, ptr(out), stream()),
              "cascade_merge")
        return out
