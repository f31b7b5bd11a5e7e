"""Sliding-window inference on the native path (reference trainer.py:17-98, `predict_per_patch`).

Same call, same window placement and the same merge arithmetic as the reference, including what its
code does rather than what it intends:
  * the window centres come from `np.arange(start, end + 1e-8, step, dtype=np.int)` with a fractional
    step (trainer.py:38-40).  For an integer dtype numpy derives the spacing from the first two values
    cast to int, so the centres are `int(start) + i * (int(start + step) - int(start))`; the last window
    then often stops short of the far border and those voxels are never visited (0/0 = NaN ->
    class 0 in the mask, NaN in the one-hot map).  `window_centres` restates that rule explicitly
    (`np.int` is gone from numpy >= 1.24, where the reference raises AttributeError);
  * the averaged probabilities go through a second softmax before the argmax (trainer.py:93).

What runs where: every window is one forward of the model through the HIP kernels; the softmax +
accumulate and the divide + softmax + argmax + crop are two streaming HIP kernels
(`ru3d_predict_accumulate`, `ru3d_predict_merge`); the volumes `result` / `result_n` live in HBM as
[X, Y, Z, C] / [X, Y, Z] fp32 for the whole case and only the final mask crosses PCIe.
`patch_batch` windows are pushed through the network per forward (InstanceNorm is per sample, so the
result does not depend on it); the sums are still accumulated in the reference's window order.

Beyond the reference (keyword-only options of `predict_per_patch`; at their defaults the code above runs unchanged):
  * `placement='cover'`: per axis of padded length L and patch P, n = ceil((L - P) * s / P) + 1 windows with lower
    corners (i * (L - P)) // (n - 1) (`cover_origins`) - the first at 0, the last at L - P, steps of at most
    ceil(P / s) - so every voxel is predicted and nothing comes back NaN; the final crop uses `pad_offset`, so the
    result sits on the input's own grid (no one-voxel shift for an odd pad);
  * `weighting='gaussian'`: a window's probabilities are weighted by (g_x[a] * g_y[j]) * g_z[k], g from
    `gaussian_profile` (float64 on the host, rounded to fp32, uploaded once); `cnt` sums the same weights;
  * `mirror_axes`: every window is predicted once per subset of the axes (`mirror_subsets`: by size, then
    lexicographic, the empty set first), the input mirrored on the way into the model and the probabilities
    mirrored back on the way into `acc`, both by index arithmetic inside `ru3d_predict_gather` /
    `ru3d_predict_accumulate_weighted` - no flipped copies of inputs or logits exist;
  * `model` may be a list: all members add into the same `acc` / `cnt`;
  * `groups`: the channels are overlapping label groups (loss.GroupHybirdLoss) - every window goes through
    `ru3d_predict_accumulate_groups` (an independent sigmoid per channel, on the reference route and on the blended one)
    and the label map is decoded by `ru3d_predict_merge_groups` (the last group above its threshold wins, 0 otherwise).
Summation order (fixed): models in list order, outermost; inside a model the windows in loop order (x outer, z inner);
inside a window the mirror subsets in `mirror_subsets` order.  Every term is one accumulate launch on one stream and a
launch owns each voxel of its window once, so there are no atomics and no races; `patch_batch` only decides how many
consecutive terms share a forward, never the order of the sums: the result is bit-identical for every `patch_batch`.
"""
import ctypes
import itertools
import math

import numpy as np
import torch

import _native as N
from _native import check, ptr, stream

try:
    from tqdm import tqdm
except Exception:  # pragma: no cover
    tqdm = None


def padded_shape(shape, patch_size):
    """`pad(input, patch_size)` (transform.py:386-389): every axis at least as long as the patch."""
    return tuple(max(int(shape[i]), int(patch_size[i])) for i in range(3))


def pad_offset(orig, full):
    """Where `pad` puts the case inside the padded volume: crop_pad's centred box starts at
    (orig - full) // 2 <= 0 and that many voxels are padded in front (transform.py:401-432)."""
    return tuple(-((int(orig[i]) - int(full[i])) // 2) for i in range(3))


def crop_offset(orig, full):
    """Where the final `crop_pad(result, original_shape)` cuts (trainer.py:98): (full - orig) // 2.  For an
    odd difference this is one voxel less than `pad_offset` - the reference returns such a case shifted
    by one voxel along that axis, and so does this function."""
    return tuple((int(full[i]) - int(orig[i])) // 2 for i in range(3))


def window_centres(length, patch, step_per_patch):
    """Window centres along one axis of (padded) length `length` (trainer.py:29-40)."""
    start = patch // 2
    end = length - patch // 2
    num_steps = math.ceil((end - start) / (patch / step_per_patch))
    step = (end - start) / (num_steps + 1e-8)
    if step == 0:
        step = 9999999
    # np.arange(start, end + 1e-8, step, dtype=int): length from the float arguments, spacing from the
    # first two values truncated to int
    count = int(math.ceil((end + 1e-8 - start) / step))
    delta = int(start + step) - int(start)
    return [int(start) + i * delta for i in range(max(count, 0))]


def window_origins(shape, patch_size, step_per_patch):
    """Lower corners of all windows in the reference's loop order (x outer, z inner; trainer.py:55-67)."""
    axes = [window_centres(shape[i], patch_size[i], step_per_patch) for i in range(3)]
    return [(x - patch_size[0] // 2, y - patch_size[1] // 2, z - patch_size[2] // 2)
            for x in axes[0] for y in axes[1] for z in axes[2]], [len(a) for a in axes]


PLACEMENTS = ('reference', 'cover')
WEIGHTINGS = ('uniform', 'gaussian')


def cover_origins(length, patch, step_per_patch):
    """Lower corners of the windows along one axis of padded length `length` >= `patch` under placement='cover':
    n = ceil((length - patch) * step_per_patch / patch) + 1 windows at (i * (length - patch)) // (n - 1), integers
    throughout.  First corner 0, last corner length - patch, steps of at most ceil(patch / step_per_patch)."""
    length, patch, s = int(length), int(patch), int(step_per_patch)
    if patch < 1 or s < 1 or length < patch:
        raise ValueError("cover_origins: need length >= patch >= 1 and step_per_patch >= 1, got (%d, %d, %d)"
                         % (length, patch, s))
    span = length - patch
    n = -((-span * s) // patch) + 1
    if n == 1:
        return [0]
    return [(i * span) // (n - 1) for i in range(n)]


def cover_window_origins(shape, patch_size, step_per_patch):
    """`window_origins` for placement='cover': same loop order (x outer, z inner)."""
    axes = [cover_origins(shape[i], patch_size[i], step_per_patch) for i in range(3)]
    return [(x, y, z) for x in axes[0] for y in axes[1] for z in axes[2]], [len(a) for a in axes]


def gaussian_profile(P, sigma_scale=0.125):
    """Per-axis blending weights of a window of `P` voxels: g[i] = exp(-0.5 * ((i - (P - 1) / 2) / (sigma_scale * P))**2),
    computed in float64 and rounded to float32.  The smallest product of three (a window corner) stays a normal fp32
    number for sigma_scale = 1/8 and is neither clamped nor flushed."""
    P = int(P)
    sigma_scale = float(sigma_scale)
    if P < 1 or not sigma_scale > 0:
        raise ValueError("gaussian_profile: need P >= 1 and sigma_scale > 0, got (%d, %r)" % (P, sigma_scale))
    i = np.arange(P, dtype=np.float64)
    return np.exp(-0.5 * ((i - (P - 1) / 2.0) / (sigma_scale * P)) ** 2).astype(np.float32)


def mirror_subsets(axes):
    """The mirror variants of a window for `mirror_axes`: every subset of the axes as a sorted tuple, ordered by size,
    then lexicographically; the empty set (the plain window) first."""
    axes = sorted(int(a) for a in axes)
    return [c for r in range(len(axes) + 1) for c in itertools.combinations(axes, r)]


_DEFAULTS = dict(placement='reference', weighting='uniform', mirror_axes=(), sigma_scale=0.125)


class Blended:
    """A model, or a list of models, together with blending options: accepted wherever a driver takes a model.  The
    drivers whose parameter lists are fixed (cascade_predict_case, cascade_predict, batch_cascade_predict) receive the
    options this way, per stage; for the others it is the same as passing the keywords.  `parameters()` and
    `out_channels` are the first member's, which is what the drivers ask a model for."""

    def __init__(self, model, *, placement='reference', weighting='uniform', mirror_axes=(), sigma_scale=0.125):
        if isinstance(model, Blended):
            raise ValueError("Blended: model is already a Blended")
        self.options = dict(placement=placement, weighting=weighting, mirror_axes=tuple(mirror_axes),
                            sigma_scale=sigma_scale)
        self.models, _ = check_options(model, who="Blended", **self.options)

    def parameters(self):
        return self.models[0].parameters()

    @property
    def out_channels(self):
        return self.models[0].out_channels


def _model_list(model, who="predict_per_patch"):
    models = list(model) if isinstance(model, (list, tuple)) else [model]
    if not models:
        raise ValueError("%s: model is an empty list" % who)
    return models


def check_options(model, placement='reference', weighting='uniform', mirror_axes=(), sigma_scale=0.125,
                  who="predict_per_patch"):
    """Validate the blending options on the host, before anything touches the device.  Returns (models, mirror axes)."""
    if isinstance(model, Blended):
        raise ValueError("%s: model is a Blended; unwrap it with resolve_options" % who)
    if placement not in PLACEMENTS:
        raise ValueError("%s: placement must be one of %s, got %r" % (who, PLACEMENTS, placement))
    if weighting not in WEIGHTINGS:
        raise ValueError("%s: weighting must be one of %s, got %r" % (who, WEIGHTINGS, weighting))
    try:
        axes = tuple(mirror_axes)
    except TypeError:
        raise ValueError("%s: mirror_axes must be a sequence of axes out of (0, 1, 2), got %r" % (who, mirror_axes))
    for a in axes:
        if isinstance(a, bool) or not isinstance(a, (int, np.integer)) or not 0 <= int(a) <= 2:
            raise ValueError("%s: mirror_axes holds %r; the axes are 0, 1, 2 (X, Y, Z)" % (who, a))
    axes = tuple(int(a) for a in axes)
    if len(set(axes)) != len(axes):
        raise ValueError("%s: mirror_axes names an axis twice: %s" % (who, axes))
    if isinstance(sigma_scale, bool) or not isinstance(sigma_scale, (int, float, np.floating, np.integer)) \
            or not float(sigma_scale) > 0 or not math.isfinite(float(sigma_scale)):
        raise ValueError("%s: sigma_scale must be a finite number > 0, got %r" % (who, sigma_scale))
    models = _model_list(model, who)
    devices = [p.device for p in (next(m.parameters(), None) for m in models) if p is not None]
    if any(d != devices[0] for d in devices):
        raise ValueError("%s: the models of the ensemble live on different devices: %s"
                         % (who, ", ".join(str(d) for d in devices)))
    return models, axes


def resolve_options(model, placement='reference', weighting='uniform', mirror_axes=(), sigma_scale=0.125,
                    who="predict_per_patch"):
    """(models, options dict) of a driver call: the keywords, or - when `model` is a Blended - its options, which a
    keyword may repeat but not contradict."""
    given = dict(placement=placement, weighting=weighting, mirror_axes=mirror_axes, sigma_scale=sigma_scale)
    if isinstance(model, Blended):
        for k, v in given.items():
            if k == 'mirror_axes' and isinstance(v, (list, tuple)):
                v = tuple(v)
            if v != _DEFAULTS[k] and v != model.options[k]:
                raise ValueError("%s: %s=%r contradicts the Blended model's %s=%r" % (who, k, v, k, model.options[k]))
        given = dict(model.options)
        model = model.models
    models, axes = check_options(model, who=who, **given)
    given['mirror_axes'] = axes
    return models, given


def _group_decode(groups, group_labels, threshold, num_classes, who):
    """None without groups; otherwise the checked (K label values, K thresholds) of a driver's group arguments."""
    if groups is None:
        if group_labels is not None:
            raise ValueError("%s: group_labels without groups" % who)
        return None
    import transform
    decode = transform._checked_decode(groups, group_labels, threshold)
    if int(num_classes) != len(decode[0]):
        raise ValueError("%s: num_classes is %d but there are %d groups" % (who, num_classes, len(decode[0])))
    return decode


def _blend_windows(vol, models, num_classes, patch_size, origins, flips, tables, acc, cnt, patch_batch, bar,
                   groups=False):
    """The mirrored / weighted / ensemble window loop.  vol: dense fp32 [X, Y, Z, Cin] on the device.  Terms are
    issued in the fixed order (model, window, mirror subset); `patch_batch` consecutive terms share one forward.
    groups: the channels are label groups - an independent sigmoid each instead of the softmax."""
    accumulate, what = (N.lib.ru3d_predict_accumulate_groups, "predict_accumulate_groups") if groups else \
        (N.lib.ru3d_predict_accumulate_weighted, "predict_accumulate_weighted")
    device = vol.device
    X, Y, Z, cin = (int(v) for v in vol.shape)
    px, py, pz = patch_size
    terms = [(o, f) for o in origins for f in flips]
    gx, gy, gz = (ptr(t) for t in tables) if tables is not None else (None, None, None)
    for model in models:
        model.eval()
        for b0 in range(0, len(terms), patch_batch):
            group = terms[b0:b0 + patch_batch]
            x = N.new_act(len(group), cin, px, py, pz, torch.float32, device)
            for g0 in range(0, len(group), N.PREDICT_MAX_BATCH):
                part = group[g0:g0 + N.PREDICT_MAX_BATCH]
                flat = (ctypes.c_int32 * (4 * len(part)))(*[v for (o, f) in part for v in (o[0], o[1], o[2], f)])
                d = N.desc(x[g0:g0 + len(part)])
                check(N.lib.ru3d_predict_gather(ptr(vol), X, Y, Z, cin, flat, len(part), ctypes.byref(d), stream()),
                      "predict_gather")
            logits = model(x)
            if logits.shape[1] != num_classes:
                raise ValueError("predict_per_patch: model returns %d classes, num_classes is %d"
                                 % (logits.shape[1], num_classes))
            logits = N.to_ndhwc(logits)
            d = N.desc(logits)
            for i, ((ox, oy, oz), f) in enumerate(group):
                check(accumulate(ctypes.byref(d), N.dtype_code(logits.dtype), i, f, gx, gy, gz, ptr(acc), ptr(cnt), X, Y,
                                 Z, ox, oy, oz, stream()), what)
            if bar is not None:
                bar.update(len(group))


def predict_per_patch(input, model, num_classes=3, patch_size=(96, 96, 96), step_per_patch=4, verbose=True,
                      one_hot=False, patch_batch=1, return_device=False, *,
                      groups=None, group_labels=None, threshold=0.5,
                      placement='reference', weighting='uniform', mirror_axes=(), sigma_scale=0.125):
    """input: numpy (or torch, host or device) [X, Y, Z, C_in] (the reference's W,H,D,C case layout).  Returns the
    uint8 mask [X, Y, Z] (or the float32 [X, Y, Z, num_classes] probability map when one_hot) at the input's own shape,
    as a numpy array like the reference - or as the device tensor when return_device (predict_case keeps going on
    the GPU).

    model: one model or a list / tuple of models on one HIP device (an ensemble; architectures and compute dtypes may
    differ).  placement: 'reference' (the reference's windows and crop, uncovered NaN border included) or 'cover'
    (every voxel inside a window, result on the input's own grid).  weighting: 'uniform' or 'gaussian' (centre-weighted,
    width sigma_scale * patch per axis).  mirror_axes: subset of (0, 1, 2); every window is also predicted mirrored
    along every non-empty subset of these axes.  The module docstring has the rules and the summation order.

    groups: the model was trained with the group losses (loss.GroupHybirdLoss): num_classes must equal len(groups), every
    channel goes through a sigmoid of its own (`ru3d_predict_accumulate_groups`, on both routes), one_hot returns the mean
    sigmoid probabilities [X, Y, Z, K], and the label map is decoded by `ru3d_predict_merge_groups`: channel k is on iff its
    mean probability is > threshold (a number or one per group), the voxel gets group_labels[k] (default
    transform.default_group_labels(groups)) of the last channel that is on, 0 when none is or no window reached it."""
    decode = _group_decode(groups, group_labels, threshold, num_classes, "predict_per_patch")
    models, opt = resolve_options(model, placement, weighting, mirror_axes, sigma_scale)
    placement, weighting, mirror_axes, sigma_scale = (opt[k] for k in ('placement', 'weighting', 'mirror_axes',
                                                                        'sigma_scale'))
    blended = placement != 'reference' or weighting != 'uniform' or len(mirror_axes) > 0 or len(models) > 1
    model = models[0]
    device = next(model.parameters()).device
    for m in models:
        N.require_device(next(m.parameters()), "model")
    patch_size = tuple(int(p) for p in patch_size)
    if any(p % 2 for p in patch_size):
        # the reference slices [c - p//2, c + p//2): an odd patch would feed the model p-1 voxels
        raise ValueError("predict_per_patch: patch_size must be even, got %s" % (patch_size,))
    if not torch.is_tensor(input):
        input = np.asarray(input)
    if input.ndim != 4:
        raise ValueError("predict_per_patch: expected a [X, Y, Z, C] volume, got shape %s" % (input.shape,))
    original_shape = tuple(int(s) for s in input.shape[:3])
    full = padded_shape(original_shape, patch_size)
    lo = pad_offset(original_shape, full)
    co = crop_offset(original_shape, full)
    cin = int(input.shape[3])

    # padded volume in HBM, NDHWC (= the case layout with a leading batch axis); zero padding as np.pad's default
    vol = torch.zeros((1,) + full + (cin,), dtype=torch.float32, device=device)
    vol[0, lo[0]:lo[0] + original_shape[0], lo[1]:lo[1] + original_shape[1], lo[2]:lo[2] + original_shape[2]] = \
        (input.to(device=device, dtype=torch.float32) if torch.is_tensor(input)
         else torch.from_numpy(np.ascontiguousarray(input, dtype=np.float32)).to(device))
    dense = vol[0]                                                     # [X, Y, Z, C], what the gather kernel reads
    vol = vol.permute(0, 4, 1, 2, 3)                                   # [1, C, X, Y, Z] view

    if placement == 'cover':
        origins, counts = cover_window_origins(full, patch_size, step_per_patch)
        co = lo                                                        # crop where pad put the case: no shift
    else:
        origins, counts = window_origins(full, patch_size, step_per_patch)
    for (ox, oy, oz) in origins:
        if ox < 0 or oy < 0 or oz < 0 or ox + patch_size[0] > full[0] or oy + patch_size[1] > full[1] \
                or oz + patch_size[2] > full[2]:
            raise ValueError("predict_per_patch: window at %s leaves the %s volume" % ((ox, oy, oz), full))
    if verbose:
        print('Image Shape: {} Patch Size: {}'.format(full, patch_size))
        print('X step: %d Y step: %d Z step: %d' % tuple(counts))

    acc = torch.zeros(full + (num_classes,), dtype=torch.float32, device=device)
    cnt = torch.zeros(full, dtype=torch.float32, device=device)
    px, py, pz = patch_size
    patch_batch = max(1, int(patch_batch))
    flips = [sum(1 << a for a in sub) for sub in mirror_subsets(mirror_axes)]
    total = len(origins) * len(flips) * len(models) if blended else len(origins)
    bar = tqdm(total=total) if (verbose and tqdm is not None) else None
    model.eval()
    with torch.no_grad():
        if blended:
            tables = None
            if weighting == 'gaussian':
                tables = [torch.from_numpy(gaussian_profile(p, sigma_scale)).to(device) for p in patch_size]
            _blend_windows(dense, models, num_classes, patch_size, origins, flips, tables, acc, cnt, patch_batch, bar,
                           groups=decode is not None)
        for b0 in (() if blended else range(0, len(origins), patch_batch)):
            group = origins[b0:b0 + patch_batch]
            x = N.new_act(len(group), cin, px, py, pz, torch.float32, device)
            for i, (ox, oy, oz) in enumerate(group):
                x[i].copy_(vol[0, :, ox:ox + px, oy:oy + py, oz:oz + pz])
            logits = model(x)
            if logits.shape[1] != num_classes:
                raise ValueError("predict_per_patch: model returns %d classes, num_classes is %d"
                                 % (logits.shape[1], num_classes))
            logits = N.to_ndhwc(logits)
            d = N.desc(logits)
            for i, (ox, oy, oz) in enumerate(group):
                if decode is not None:
                    check(N.lib.ru3d_predict_accumulate_groups(ctypes.byref(d), N.dtype_code(logits.dtype), i, 0, None,
                                                               None, None, ptr(acc), ptr(cnt), full[0], full[1], full[2],
                                                               ox, oy, oz, stream()), "predict_accumulate_groups")
                    continue
                check(N.lib.ru3d_predict_accumulate(ctypes.byref(d), N.dtype_code(logits.dtype), i, ptr(acc),
                                                    ptr(cnt), full[0], full[1], full[2], ox, oy, oz, stream()),
                      "predict_accumulate")
            if bar is not None:
                bar.update(len(group))
    if bar is not None:
        bar.close()
    if verbose:
        print('Merging all patchs...')
    sx, sy, sz = original_shape
    if one_hot:
        out = torch.empty(original_shape + (num_classes,), dtype=torch.float32, device=device)
    else:
        out = torch.empty(original_shape, dtype=torch.uint8, device=device)
    N.note_device(acc.device)
    if decode is not None and not one_hot:
        labels, thr = decode
        check(N.lib.ru3d_predict_merge_groups(ptr(acc), ptr(cnt), full[0], full[1], full[2], num_classes,
                                              (ctypes.c_int32 * num_classes)(*labels),
                                              (ctypes.c_float * num_classes)(*[float(t) for t in thr]), co[0], co[1],
                                              co[2], sx, sy, sz, ptr(out), stream()), "predict_merge_groups")
        return out if return_device else out.cpu().numpy()
    check(N.lib.ru3d_predict_merge(ptr(acc), ptr(cnt), full[0], full[1], full[2], num_classes, co[0], co[1], co[2],
                                   sx, sy, sz, 1 if one_hot else 0, ptr(out), stream()), "predict_merge")
    return out if return_device else out.cpu().numpy()


# --------------------------------------------------------------------------- whole-case inference (trainer.py:101-133)
def _zoomed_shape(shape, scale):
    """Output shape of scipy.ndimage.zoom for an input shape and per-axis factors."""
    return tuple(int(round(s * z)) for s, z in zip(shape, scale))


def resample_normalize_image(vol, out_shape, stats):
    """fp32 HIP volume [X, Y, Z, C] -> [x, y, z, len(stats)]: the order-1 zoom kernel, then per channel the clip to
    [pct_00_5, pct_99_5] and (x - mean) / (std + 1e-8) (reference data.py:222-283).  Shared by predict_case and
    data.resample_normalize_case."""
    import augment
    vol = augment.resample_image(vol, out_shape)
    for c, s in enumerate(stats):
        vol[..., c].clamp_(float(s['pct_00_5']), float(s['pct_99_5'])).sub_(float(s['mean'])).div_(float(s['std']) + 1e-8)
    return vol[..., :len(stats)]


def predict_case(case, model, target_spacing, normalize_stats, num_classes=3, patch_size=(96, 96, 96),
                 step_per_patch=4, verbose=True, one_hot=False, patch_batch=1, return_device=False, *,
                 groups=None, group_labels=None, threshold=0.5,
                 placement='reference', weighting='uniform', mirror_axes=(), sigma_scale=0.125):
    """reference trainer.py:101-133: resample the case to `target_spacing` and normalise it (data.py:222-283), run the
    sliding-window prediction, resize the prediction back to the case's shape.  Everything between the upload of the
    image and the download of the prediction runs on the device: the two resamplings are the order-1 zoom kernel of
    the augmentation path (label rule included), the sliding window is predict_per_patch.  `case['image']` may already
    be a HIP tensor (no upload), and `return_device` leaves `case['pred']` in HBM (no download): the cascade chains its
    stages that way.  `model` may be a list; placement / weighting / mirror_axes / sigma_scale and groups / group_labels
    / threshold go to predict_per_patch."""
    import augment
    _group_decode(groups, group_labels, threshold, num_classes, "predict_case")
    models, opt = resolve_options(model, placement, weighting, mirror_axes, sigma_scale, "predict_case")
    device = next(models[0].parameters()).device
    image = case['image'] if torch.is_tensor(case['image']) else np.asarray(case['image'])
    if image.ndim == 3:
        image = image[..., None]
    orig_shape = tuple(int(s) for s in image.shape[:-1])
    affine = np.asarray(case['affine'], dtype=np.float64)
    stats = normalize_stats if isinstance(normalize_stats, list) else [normalize_stats]
    if verbose:
        print('Resampling the case for prediction...')
    spacing = np.array([np.linalg.norm(affine[i, :3]) for i in range(3)])
    scale = spacing / np.array(target_spacing, dtype=np.float64)
    if torch.is_tensor(image):
        vol = image.to(device=device, dtype=torch.float32).contiguous()
    else:
        vol = torch.from_numpy(np.ascontiguousarray(image, dtype=np.float32)).to(device)
    vol = resample_normalize_image(vol, _zoomed_shape(orig_shape, scale), stats)
    if verbose:
        print('Predicting the case...')
    pred = predict_per_patch(vol, models, num_classes, patch_size, step_per_patch, verbose, one_hot,
                             patch_batch=patch_batch, return_device=True, groups=groups, group_labels=group_labels,
                             threshold=threshold, **opt)
    if verbose:
        print('Resizing the case to origial shape...')
    if one_hot:
        out = augment.resample_image(pred, orig_shape)
    else:
        out = augment.resample_label(pred, orig_shape).to(torch.uint8)
    case['pred'] = out if return_device else out.cpu().numpy()
    case['affine'] = affine
    if verbose:
        print('All done!')
    return case
