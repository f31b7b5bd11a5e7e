"""Dataset preparation on the device (csrc/prepare.hip).

The host code these replace when a case lives in HBM: the `np.where(channel > air)` index arrays of `orient_crop_case`
(reference data.py:150-160), the boolean-mask gather `image[label > 0][::10]` of `analyze_cases` (data.py:365-372) and
the `np.median / np.percentile / np.mean / np.std / np.min / np.max` over the pooled sample (data.py:378-388).  The box,
the sample (values and order) and every order statistic are numpy's, bit for bit; mean and standard deviation are
accumulated in float64 in a fixed order.  There is no host fallback in here: every function wants HIP tensors.
"""
import ctypes

import numpy as np
import torch

import _native as N
from _native import check, ptr, stream
from components import MAX_VOXELS


def _case_image(image, what):
    """fp32 contiguous [X, Y, Z, C] HIP tensor of a case image (a 3-D volume gets its channel axis)."""
    if not torch.is_tensor(image):
        raise ValueError("%s: expected a HIP tensor, got %s" % (what, type(image).__name__))
    N.require_device(image, what)
    if image.dim() == 3:
        image = image[..., None]
    if image.dim() != 4:
        raise ValueError("%s: expected a [X, Y, Z, C] image, got shape %s" % (what, tuple(image.shape)))
    if image.numel() == 0 or image[..., 0].numel() >= MAX_VOXELS:
        raise ValueError("%s: a volume of shape %s is not supported (1 .. 2**31 - 1 voxels)" % (what, tuple(image.shape)))
    return image.to(torch.float32).contiguous()


def _flat_values(values, what):
    if not torch.is_tensor(values):
        raise ValueError("%s: expected a HIP tensor, got %s" % (what, type(values).__name__))
    N.require_device(values, what)
    if values.dtype != torch.float32:
        raise ValueError("%s: expected float32 values, got %s" % (what, values.dtype))
    values = values.contiguous().reshape(-1)
    if values.numel() == 0:
        raise ValueError("%s: no values" % what)
    return values


def threshold_bbox(image, threshold):
    """image: HIP tensor [X, Y, Z, C] (or [X, Y, Z]).  Returns (bbox, count): bbox is the int64 numpy array (3, 2) of the
    smallest and the largest index, per axis, of a voxel with any channel > threshold (the upper bound is the last index
    itself, as orient_crop_case records it), count the number of such voxels.  No voxel above the threshold: ValueError,
    as numpy's `min` of an empty array raises."""
    img = _case_image(image, "threshold_bbox")
    X, Y, Z, C = (int(s) for s in img.shape)
    box = torch.empty(6, dtype=torch.int32, device=img.device)
    count = torch.empty(1, dtype=torch.int64, device=img.device)
    check(N.lib.ru3d_threshold_bbox(ptr(img), X, Y, Z, C, float(threshold), ptr(box), ptr(count), stream(img.device)),
          "threshold_bbox")
    n = int(count.item())
    if n == 0:
        raise ValueError("threshold_bbox: no voxel above the threshold %r" % (threshold,))
    return box.cpu().numpy().astype(np.int64).reshape(3, 2), n


def _label_volume(label, shape, what):
    if not torch.is_tensor(label):
        raise ValueError("%s: expected a HIP tensor as the label, got %s" % (what, type(label).__name__))
    if tuple(label.shape) != tuple(shape):
        raise ValueError("%s: label of shape %s for an image of %s" % (what, tuple(label.shape), tuple(shape)))
    if label.dtype == torch.bool:
        label = label.contiguous().view(torch.uint8)
    elif label.dtype not in (torch.uint8, torch.int64):
        label = label.to(torch.int64)
    return label.contiguous(), (N.LABEL_U8 if label.dtype == torch.uint8 else N.LABEL_I64)


def _masked_sample_call(img, lab, code, channel, stride, out, count):
    X, Y, Z, C = (int(s) for s in img.shape)
    ws = N.workspace(N.lib.ru3d_masked_sample_workspace_bytes(X, Y, Z), img.device)
    N.note_device(img.device)
    check(N.lib.ru3d_masked_sample(ptr(img) if out is not None else None, X, Y, Z, C, int(channel), ptr(lab), code,
                                   int(stride), ptr(out), out.numel() if out is not None else 0, ptr(count), ptr(ws),
                                   ws.numel(), stream()), "masked_sample")
    return int(count.item())


def masked_sample(image, label, channel, stride=10, out=None):
    """`image[..., channel][label > 0][::stride]` of HIP tensors in numpy's element order, as a 1-D fp32 HIP tensor.
    With `out` (1-D contiguous fp32 HIP tensor, e.g. the free tail of a pooled buffer) the samples are written to its
    front and the filled view is returned; an `out` that is too small raises ValueError and nothing is written past its
    end.  Without it the call runs twice: count, then fill."""
    img = _case_image(image, "masked_sample")
    C = int(img.shape[3])
    if not 0 <= int(channel) < C:
        raise ValueError("masked_sample: channel %r of %d" % (channel, C))
    if int(stride) < 1:
        raise ValueError("masked_sample: stride %r (>= 1)" % (stride,))
    lab, code = _label_volume(label, img.shape[:3], "masked_sample")
    if lab.device != img.device:
        raise ValueError("masked_sample: image on %s, label on %s" % (img.device, lab.device))
    count = torch.empty(1, dtype=torch.int64, device=img.device)
    if out is None:
        n = _masked_sample_call(img, lab, code, channel, stride, None, count)
        out = torch.empty(n, dtype=torch.float32, device=img.device)
    elif not torch.is_tensor(out) or out.dtype != torch.float32 or out.dim() != 1 or not out.is_contiguous() \
            or out.device != img.device:
        raise ValueError("masked_sample: out must be a contiguous 1-D float32 tensor on %s" % (img.device,))
    n = _masked_sample_call(img, lab, code, channel, stride, out if out.numel() else None, count)
    if n > out.numel():
        raise ValueError("masked_sample: %d samples for a buffer of %d" % (n, out.numel()))
    return out[:n]


class SamplePool:
    """The pooled intensity sample of analyze_cases, resident in HBM: one fp32 buffer that the cases' samples are
    appended to (count, grow geometrically when needed, fill) and that the statistics kernels read once at the end."""

    def __init__(self, device, capacity=1 << 20):
        self.buffer = torch.empty(int(capacity), dtype=torch.float32, device=device)
        self.size = 0

    def append(self, image, label, channel, stride):
        img = _case_image(image, "SamplePool.append")
        lab, code = _label_volume(label, img.shape[:3], "SamplePool.append")
        count = torch.empty(1, dtype=torch.int64, device=img.device)
        n = _masked_sample_call(img, lab, code, channel, stride, None, count)
        if self.size + n > self.buffer.numel():
            grown = torch.empty(max(2 * self.buffer.numel(), self.size + n), dtype=torch.float32, device=self.buffer.device)
            grown[:self.size] = self.buffer[:self.size]
            self.buffer = grown
        if n:
            masked_sample(img, lab, channel, stride, out=self.buffer[self.size:self.size + n])
        self.size += n
        return n

    def values(self):
        return self.buffer[:self.size]


def order_statistics(values, ranks):
    """The `ranks`-th smallest (zero-based, at most 8 of them) of a fp32 HIP tensor, as a float32 numpy array equal to
    `np.sort(values)[ranks]`.  Nothing is sorted: a radix select reads the values four times."""
    v = _flat_values(values, "order_statistics")
    ranks = [int(r) for r in np.atleast_1d(ranks)]
    if not 1 <= len(ranks) <= N.ORDER_STATS_MAX_RANKS:
        raise ValueError("order_statistics: %d ranks (1 .. %d)" % (len(ranks), N.ORDER_STATS_MAX_RANKS))
    for r in ranks:
        if not 0 <= r < v.numel():
            raise ValueError("order_statistics: rank %d of %d values" % (r, v.numel()))
    out = torch.empty(len(ranks), dtype=torch.float32, device=v.device)
    ws = N.workspace(N.lib.ru3d_order_stats_workspace_bytes(), v.device)
    N.note_device(v.device)
    check(N.lib.ru3d_order_stats(ptr(v), v.numel(), (ctypes.c_int64 * len(ranks))(*ranks), len(ranks), ptr(out), ptr(ws),
                                 ws.numel(), stream()), "order_stats")
    return out.cpu().numpy()


def moments(values):
    """(n, min, max, mean, std) of a fp32 HIP tensor as a float64 numpy array; std is the population one (ddof = 0)."""
    v = _flat_values(values, "moments")
    out = torch.empty(5, dtype=torch.float64, device=v.device)
    ws = N.workspace(N.lib.ru3d_moments_workspace_bytes(), v.device)
    N.note_device(v.device)
    check(N.lib.ru3d_moments(ptr(v), v.numel(), ptr(out), ptr(ws), ws.numel(), stream()), "moments")
    return out.cpu().numpy()


_NUMPY2 = int(np.__version__.split('.')[0]) >= 2


def _quantile_plan(n, q):
    """np.percentile(float32 values, q) with the default 'linear' method, up to the values themselves: the two ranks it
    reads and the weight between them, computed with numpy's own expressions (numpy/lib/_function_base_impl.py
    `_quantile`, `_get_indexes`, `_get_gamma`) so that the arithmetic types are the installed numpy's - numpy >= 2 divides
    q by float32(100) and keeps the virtual index (n - 1) * q in float32, numpy 1.x works in float64."""
    quantile = np.asanyarray(np.true_divide(q, np.float32(100) if _NUMPY2 else 100))
    virtual = np.asanyarray((n - 1) * quantile)
    previous = np.asanyarray(np.floor(virtual))
    lo, hi = int(previous), int(previous) + 1
    if virtual >= n - 1:
        lo = hi = n - 1
    if virtual < 0:
        lo = hi = 0
    gamma = np.asanyarray(np.asanyarray(virtual - previous), dtype=virtual.dtype)
    return lo, hi, gamma


def _lerp(a, b, t):
    """numpy's `_lerp` (same file) on two float32 scalars and the weight of _quantile_plan."""
    a, b = np.float32(a), np.float32(b)
    diff = np.subtract(b, a)
    out = np.asanyarray(np.add(a, diff * t))
    np.subtract(b, diff * (1 - t), out=out, where=t >= 0.5, casting='unsafe', dtype=type(out.dtype))
    return out[()]


def intensity_statistics(values):
    """The reference's statistics of one modality (data.py:378-388) over a fp32 HIP tensor: {'median', 'mean', 'std',
    'min', 'max', 'pct_00_5', 'pct_99_5'} as Python floats.  Median and percentiles interpolate, on the host, between the
    two neighbouring order statistics the device selects."""
    v = _flat_values(values, "intensity_statistics")
    if bool(torch.isnan(v).any().item()):
        raise ValueError("intensity_statistics: the values contain NaN")
    n = v.numel()
    plan = {'pct_00_5': _quantile_plan(n, 0.5), 'pct_99_5': _quantile_plan(n, 99.5)}
    middle = ((n - 1) // 2, n // 2)                      # np.median: the mean of the two middle values, in float32
    ranks = sorted({r for lo, hi, _ in plan.values() for r in (lo, hi)} | set(middle))
    picked = dict(zip(ranks, order_statistics(v, ranks)))
    _, lo, hi, mean, std = moments(v)
    stats = {name: float(_lerp(picked[a], picked[b], t)) for name, (a, b, t) in plan.items()}
    stats['median'] = float(np.mean(np.array([picked[r] for r in middle], dtype=np.float32)))
    stats.update(mean=float(mean), std=float(std), min=float(lo), max=float(hi))
    return {k: stats[k] for k in ('median', 'mean', 'std', 'min', 'max', 'pct_00_5', 'pct_99_5')}
