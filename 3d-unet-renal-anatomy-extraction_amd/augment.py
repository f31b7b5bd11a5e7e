"""On-device patch sampling + augmentation: the reference's training transform chain as HIP kernels.

`DeviceAugment` replaces, for volumes that live in HBM,

    Compose([RandomRescaleCrop(scale, patch, crop_mode=..., crop_margin=..., enforce_label_indices=...),
             RandomMirror(p_per_axis), RandomContrast(c), RandomBrightness(b), RandomGamma(g), ToTensor()])

of the training scripts (reference nb_train_iia.py:30-39; classes transform.py:573-652, 279-301, 196-259, 156-163).
At ~10^8 voxels/s per GPU the reference's two DataLoader workers running scipy.ndimage.zoom cannot feed one device; here
a patch costs three small kernels (csrc/augment.hip) and never leaves the GPU.

The random numbers are drawn on the HOST from numpy's global generator in exactly the reference's order (one uniform for
the scale, one randint per axis with room for the crop corner - again for every retry of enforce_label_indices -, one
uniform per mirror axis, one uniform per intensity op), so `np.random.seed(s)` reproduces the CPU pipeline's patch.

`rotation`, `elastic_spacing` and `elastic_magnitude` switch the resampling to a free-form spatial transform (rotation
about the crop box's centre, the same per-axis zoom, cubic B-spline elastic deformation; geometry and draw order: module
`spatial`, kernel: spatial_kernel in csrc/augment.hip).  `transform.RandomSpatialCrop` is its numpy twin.  Left at None
they change nothing: the same draws, the same C calls, the same bits.

`noise`, `blur` and `low_res` add Gaussian noise, Gaussian blur and simulated low resolution between the resampling and
the intensity chain (semantics, draw order and numpy twins: module `degrade`; kernels: csrc/degrade.hip).  A patch on
which one of them applies takes three C calls - the resampling with the intensity flags cleared, ru3d_augment_degrade,
ru3d_augment_intensity on the statistics of the degraded image; a patch on which none applies, and every patch when the
three keywords are None, takes the one call it always took.

`oversample_foreground` places the crop box, with that probability per patch, on a voxel drawn from the case's
class-location index (`DeviceCase.class_index` -> `ClassIndex`, kernel: csrc/locations.hip; rule, draw order and numpy
twin: module `locations`).  It replaces the rejection loop of `enforce_label_indices`, which launches the presence
kernel and reads its mask back once per try: the index is built once per case, and from then on a forced patch is the C
calls of any other patch with no transfer to the host.  `data.DeviceCaseDataset` keeps indexed cases resident for the
Trainer.  Left at None it changes nothing.
"""
import ctypes

import numpy as np
import torch

import _native as N
import degrade
import locations as fg
import spatial
from _native import check, ptr, stream


def _range(v):
    if isinstance(v, float):
        assert 0 <= v <= 1, "If range is a single number, it must be non negative"
        return [1 - v, 1 + v]
    return list(v)


class DeviceCase:
    """A case resident in HBM: image fp32 [X, Y, Z, C] (channels last, the reference's case layout, data.py) and label
    [X, Y, Z] uint8 / int64.  Built once per case; patches are cut from it on the device."""

    def __init__(self, image, label=None, device="cuda"):
        img = torch.as_tensor(np.ascontiguousarray(image) if isinstance(image, np.ndarray) else image)
        if img.dim() == 3:
            img = img[..., None]
        self.image = img.to(device=device, dtype=torch.float32).contiguous()
        self.label = None
        self._index = None
        if label is not None:
            lab = torch.as_tensor(np.ascontiguousarray(label) if isinstance(label, np.ndarray) else label)
            if lab.dtype not in (torch.uint8, torch.int64):
                lab = lab.to(torch.int64)
            self.label = lab.to(device).contiguous()
            if tuple(self.label.shape) != tuple(self.image.shape[:3]):
                raise ValueError("label %s does not match image %s" % (tuple(self.label.shape), tuple(self.image.shape)))

    @property
    def shape(self):
        return tuple(self.image.shape)

    def class_index(self, max_per_class=10000):
        """The ClassIndex of the label, built on first use and kept; another max_per_class builds it again."""
        if self.label is None:
            raise ValueError("class_index: the case has no label")
        max_per_class = fg.check_max_locations(max_per_class)
        if self._index is None or self._index.max_per_class != max_per_class:
            self._index = ClassIndex(self.label, max_per_class)
        return self._index


class ClassIndex:
    """Where the voxels of every class 0 .. 31 of a device label volume [X, Y, Z] are (ru3d_class_index; the contract
    and its numpy twin: module `locations`).  counts: numpy int64 [32]; boxes: numpy int32 [32, 6], (x0, x1, y0, y1, z0,
    z1) with the high end exclusive; device_locations: int32 device tensor [32, max_per_class], -1 behind the entries of a
    row.  One call, then one download of counts and boxes and one of the rows of the classes >= 1 that are present (what
    the sampler draws from); the row of class 0 comes down when it is first asked for."""

    def __init__(self, label, max_per_class=10000):
        self.max_per_class = m = fg.check_max_locations(max_per_class)
        if label.dtype not in (torch.uint8, torch.int64) or label.dim() != 3 or not label.is_contiguous():
            raise ValueError("ClassIndex: a contiguous uint8 or int64 device volume [X, Y, Z]")
        N.require_device(label, "the label")
        dev = label.device
        x, y, z = (int(v) for v in label.shape)
        classes = N.CLASS_INDEX_CLASSES
        # counts and boxes share one buffer: one copy brings both to the host
        head = torch.empty(classes * (2 + 6), dtype=torch.int32, device=dev)
        self.device_locations = torch.empty((classes, m), dtype=torch.int32, device=dev)
        ws = N.workspace(N.lib.ru3d_class_index_workspace_bytes(x, y, z), dev)
        code = N.LABEL_U8 if label.dtype == torch.uint8 else N.LABEL_I64
        N.note_device(dev)
        check(N.lib.ru3d_class_index(ptr(label), code, x, y, z, m, ptr(head), ptr(head[2 * classes:]),
                                     ptr(self.device_locations), ptr(ws), ws.numel(), stream()), "class_index")
        host = head.cpu().numpy()
        self.counts = host[:2 * classes].view(np.int64).copy()
        self.boxes = host[2 * classes:].reshape(classes, 6).copy()
        present = self.classes()
        self._rows = {}
        if present:
            rows = self.device_locations[present].cpu().numpy()
            for c, row in zip(present, rows):
                self._rows[c] = row[:min(int(self.counts[c]), m)].copy()

    def classes(self):
        """The label values >= 1 present in the case, ascending."""
        return [c for c in range(1, len(self.counts)) if self.counts[c] > 0]

    def locations(self, c):
        """numpy int32 [min(counts[c], max_per_class)]: linear indices (x * Y + y) * Z + z of voxels of class c."""
        c = int(c)
        if c not in self._rows:
            self._rows[c] = self.device_locations[c, :min(int(self.counts[c]), self.max_per_class)].cpu().numpy()
        return self._rows[c]


class DeviceAugment:
    def __init__(self, scale=0.1, crop_size=128, crop_mode="random", crop_margin=0, enforce_label_indices=(),
                 image_pad_cval=0, label_pad_cval=0, mirror_p=(0.5, 0.5, 0.5), contrast=0.1, brightness=0.1,
                 gamma=0.1, rng=None, rotation=None, elastic_spacing=None, elastic_magnitude=None,
                 oversample_foreground=None, foreground_classes=None, max_locations=10000, noise=None, blur=None,
                 low_res=None):
        """Arguments as the reference classes take them; contrast / brightness / gamma = None switches the op off,
        mirror_p = None the mirror.  rng: an object with numpy's `uniform` / `randint` (default: numpy's global one).

        rotation: None | r (each axis uniform in [-r, r] radians) | three (lo, hi) pairs, about x, y, z.
        elastic_spacing: control spacing of the deformation lattice in patch voxels (an int or three, >= 4) and
        elastic_magnitude: (lo, hi) in voxels - every control vector's components are uniform in [-m, m], m uniform in
        [lo, hi]; both or neither.  With any of the three set, the patch is cut *around* the drawn crop box, not equal
        to it: the box gives the centre and the zoom, enforce_label_indices and the label rule's class count test the
        axis-aligned box, and what the rotated or deformed patch reaches outside the volume reads the pad constants.

        noise, blur, low_res: None | (p, (lo, hi)) - with probability p per patch, Gaussian noise of a variance uniform
        in [lo, hi], a Gaussian blur of a sigma (voxels, one for the three axes) uniform in [lo, hi], a round trip through
        a grid of zoom uniform in [lo, hi] (0 < lo <= hi <= 1) voxels per voxel.  The usual recipe is noise
        (0.1, (0, 0.1)), blur (0.2, (0.5, 1.0)), low_res (0.25, (0.5, 1.0)).  The blur reaches int(4 sigma + 0.5) voxels
        to either side: at most 16 and at most the smallest patch extent.

        oversample_foreground: None | p in (0, 1] - with probability p per patch the crop box is placed on a voxel drawn
        from the case's class-location index (DeviceCase.class_index(max_locations), built once per case) instead of
        at random; foreground_classes: the label values (1 .. 31) to draw from, None = every value >= 1 the case holds;
        values a case lacks are skipped for it, and a case with none of them gets the random box.  Rule and draw order:
        module `locations`.  This is what replaces enforce_label_indices (the two exclude each other): no retry, no
        readback - after the first patch of a case a forced patch is the C calls of any other patch."""
        assert crop_mode in ("center", "random"), "crop mode must be either center or random"
        self.scale = _range(scale)
        self.crop_size = crop_size
        self.crop_mode = crop_mode
        self.crop_margin = crop_margin
        self.enforce = [enforce_label_indices] if isinstance(enforce_label_indices, int) else list(enforce_label_indices)
        self.image_pad_cval, self.label_pad_cval = float(image_pad_cval), int(label_pad_cval)
        self.mirror_p = mirror_p
        self.contrast = None if contrast is None else _range(contrast)
        self.brightness = None if brightness is None else _range(brightness)
        self.gamma = None if gamma is None else _range(gamma)
        self.rng = rng if rng is not None else np.random
        self.rotation = spatial.check_rotation(rotation)
        self.elastic = spatial.check_elastic(elastic_spacing, elastic_magnitude, self._patch())
        self.spatial = self.rotation is not None or self.elastic is not None
        self.noise = degrade.check_noise(noise)
        self.blur = degrade.check_blur(blur, self._patch())
        self.low_res = degrade.check_low_res(low_res, self._patch())
        self.degrade = self.noise is not None or self.blur is not None or self.low_res is not None
        self.oversample, self.foreground_classes, self.max_locations = fg.check_oversample(
            oversample_foreground, foreground_classes, max_locations, crop_mode, self.enforce)

    def _patch(self):
        return [self.crop_size] * 3 if not isinstance(self.crop_size, (list, tuple, np.ndarray)) \
            else [int(v) for v in self.crop_size]

    # ------------------------------------------------------------------ host side: the draws
    def _bbox(self, before, shape, margin):
        """transform.py:403-419 for the three spatial axes."""
        lo = []
        for i in range(3):
            if self.crop_mode == "random" and shape[i] - before[i] - margin[i] > margin[i]:
                lo.append(int(self.rng.randint(margin[i], shape[i] - before[i] - margin[i])))
            else:
                lo.append(int((shape[i] - before[i]) // 2))
        return lo

    def _index(self, case):
        index = case.class_index(self.max_locations)
        return index.counts, index.locations

    def _presence(self, case, lo, before, mask):
        lo_a = (ctypes.c_int32 * 3)(*lo)
        be_a = (ctypes.c_int32 * 3)(*before)
        lab = case.label
        code = N.LABEL_U8 if lab.dtype == torch.uint8 else N.LABEL_I64
        x, y, z = lab.shape
        N.note_device(lab.device)
        check(N.lib.ru3d_augment_label_presence(ptr(lab), code, x, y, z, lo_a, be_a, self.label_pad_cval, ptr(mask),
                                                stream()), "augment_label_presence")

    def sample(self, case, out_image=None, out_label=None):
        """One augmented patch of `case` (a DeviceCase): (image fp32 [C, px, py, pz], label int64 [px, py, pz] or None),
        written into out_image / out_label when given (slices of a batch buffer)."""
        drawn = self._draw(case)
        lattice = _upload([drawn[2][1]], case.image.device)[0] if self.elastic is not None else None
        return self._launch(case, drawn, lattice, out_image, out_label)

    def _draw(self, case):
        """Every host draw of one patch, in order (the presence kernel runs here: the enforce loop needs its answer) ->
        (PatchParams, presence mask, None | (SpatialParams, phi)), and with noise / blur / low_res configured a fourth
        entry: None | DegradeParams of the ops that apply to this patch."""
        shape = case.shape
        patch = self._patch()
        margin = [self.crop_margin] * 3 if not isinstance(self.crop_margin, (list, tuple, np.ndarray)) \
            else [int(v) for v in self.crop_margin]
        dev = case.image.device
        s = self.rng.uniform(self.scale[0], self.scale[1])
        before = [int(v) for v in np.round(np.array(patch) / s).astype(int)]
        mask = torch.empty(1, dtype=torch.int32, device=dev)
        placed = None
        if self.oversample is not None:
            placed = fg.draw_forced_box(self.rng, self.oversample, self.foreground_classes,
                                        lambda: self._index(case), before, shape, margin)
        while True:
            lo = placed if placed is not None else self._bbox(before, shape, margin)
            if case.label is None:
                break
            self._presence(case, lo, before, mask)
            if not self.enforce:
                break
            bits = int(mask.item()) & 0xffffffff          # only the enforce_label_indices loop reads back
            if all((bits >> min(int(i), 31)) & 1 for i in self.enforce):
                break
        geometry = None
        if self.spatial:
            angles, phi = spatial.draw_spatial(self.rng, self.rotation, self.elastic, patch)
            centre, matrix = spatial.patch_geometry(lo, before, patch, angles)
            sp = N.SpatialParams()
            sp.centre[:], sp.matrix[:] = centre.tolist(), matrix.reshape(-1).tolist()
            if phi is not None:
                sp.lattice[:], sp.spacing[:] = phi.shape[1:], self.elastic[0]
            geometry = (sp, phi)
        flips = [0, 0, 0]
        if self.mirror_p is not None:
            ps = self.mirror_p if isinstance(self.mirror_p, (list, tuple, np.ndarray)) else [self.mirror_p] * 3
            for i, p in enumerate(ps):
                if self.rng.uniform() < p:
                    flips[i] = 1
        pr = N.PatchParams()
        for i in range(3):
            pr.lo[i], pr.before[i], pr.patch[i], pr.flip[i] = lo[i], before[i], patch[i], flips[i]
        pr.image_cval, pr.label_cval = self.image_pad_cval, self.label_pad_cval
        pr.gamma_eps = 1e-7
        ops = degrade.draw(self.rng, self.noise, self.blur, self.low_res) if self.degrade else {}
        for name, rng_ in (("contrast", self.contrast), ("brightness", self.brightness), ("gamma", self.gamma)):
            if rng_ is not None:
                setattr(pr, "do_" + name, 1)
                setattr(pr, name, float(self.rng.uniform(rng_[0], rng_[1])))
        if self.degrade:
            return pr, mask, geometry, degrade.params(ops) if ops else None
        return pr, mask, geometry

    def _launch(self, case, drawn, lattice, out_image, out_label):
        pr, mask, geometry = drawn[:3]
        dg = drawn[3] if len(drawn) > 3 else None
        shape, patch, dev = case.shape, list(pr.patch), case.image.device
        c = shape[3]
        if out_image is None:
            out_image = torch.empty((c,) + tuple(patch), dtype=torch.float32, device=dev)
        if out_label is None and case.label is not None:
            out_label = torch.empty(tuple(patch), dtype=torch.int64, device=dev)
        if not out_image.is_contiguous() or (out_label is not None and not out_label.is_contiguous()):
            raise N.Ru3dError("DeviceAugment: output slices must be contiguous")
        full = pr
        if dg is not None:
            # the resampling without its intensity chain; the chain follows the degrade call on fresh statistics
            ws, tail = degrade.workspace(c, patch, dev)
            pr = N.PatchParams.from_buffer_copy(full)
            pr.do_contrast = pr.do_brightness = pr.do_gamma = 0
        else:
            ws = N.workspace(N.lib.ru3d_augment_workspace_bytes(*patch), dev)
        lab = case.label
        code = N.LABEL_I64 if (lab is None or lab.dtype == torch.int64) else N.LABEL_U8
        N.note_device(dev)
        if geometry is not None:
            check(N.lib.ru3d_augment_patch_spatial(ptr(case.image), ptr(lab), code, shape[0], shape[1], shape[2], c,
                                                   ctypes.byref(pr), ctypes.byref(geometry[0]), ptr(lattice),
                                                   ptr(mask) if lab is not None else None, ptr(out_image),
                                                   ptr(out_label), ptr(ws), ws.numel(), stream()),
                  "augment_patch_spatial")
        else:
            check(N.lib.ru3d_augment_patch(ptr(case.image), ptr(lab), code, shape[0], shape[1], shape[2], c,
                                           ctypes.byref(pr), ptr(mask) if lab is not None else None, ptr(out_image),
                                           ptr(out_label), ptr(ws), ws.numel(), stream()), "augment_patch")
        if dg is not None:
            total = patch[0] * patch[1] * patch[2]
            degrade.launch(out_image, dg, ws, tail)
            if full.do_contrast or full.do_brightness or full.do_gamma:
                check(N.lib.ru3d_augment_intensity(ptr(out_image), c * total, ptr(ws), (total + 255) // 256,
                                                   ctypes.byref(full), stream()), "augment_intensity")
        return out_image, out_label

    def __call__(self, case):
        """Transform interface: case = {'image': DeviceCase | array [X,Y,Z,C], 'label': ...} -> the reference's
        post-ToTensor dict with device tensors (use with num_workers=0: DataLoader workers cannot touch the GPU)."""
        dc = case["image"] if isinstance(case["image"], DeviceCase) else DeviceCase(case["image"], case.get("label"))
        img, lab = self.sample(dc)
        out = dict(case)
        out["image"], out["label"] = img, lab
        return out

    def batch(self, cases, batch_size):
        """`batch_size` patches drawn from `cases` (list of DeviceCase) with replacement, like the reference's
        RandomSampler(replacement=True) (trainer.py:549-551): {'image': [N, C, ...] fp32, 'label': [N, ...] int64}."""
        patch = self._patch()
        dev = cases[0].image.device
        c = cases[0].shape[3]
        x = torch.empty((batch_size, c) + tuple(patch), dtype=torch.float32, device=dev)
        y = torch.empty((batch_size,) + tuple(patch), dtype=torch.int64, device=dev)
        if self.elastic is None:
            for b in range(batch_size):
                case = cases[int(self.rng.randint(0, len(cases)))]
                self.sample(case, x[b], y[b])
            return {"image": x, "label": y}
        # elastic: all draws first (same order), then the lattices of the whole batch in one upload, then the patches
        picked, drawn = [], []
        for b in range(batch_size):
            picked.append(cases[int(self.rng.randint(0, len(cases)))])
            drawn.append(self._draw(picked[-1]))
        lattices = _upload([d[2][1] for d in drawn], dev)
        for b in range(batch_size):
            self._launch(picked[b], drawn[b], lattices[b], x[b], y[b])
        return {"image": x, "label": y}


def _upload(phis, device):
    """Control lattices (equal shapes) -> one device tensor [len, 3, nx, ny, nz], through pinned memory and a copy queued
    on the current stream: the host does not wait for the device."""
    staged = torch.empty((len(phis),) + phis[0].shape, dtype=torch.float32, pin_memory=True)
    for i, phi in enumerate(phis):
        staged[i].copy_(torch.from_numpy(phi))
    return staged.to(device, non_blocking=True)


# --------------------------------------------------------------------------- plain resampling (inference: predict_case)
def _resample(image, label, out_shape):
    """scipy.ndimage.zoom(order=1) of a whole device volume to `out_shape` with the augmentation kernel (crop box = the
    volume, no mirror, no intensity ops): image fp32 [X,Y,Z,C] -> fp32 [C,x,y,z]; label [X,Y,Z] -> int64 [x,y,z] by the
    reference's label rule (transform.py:47-74)."""
    ref = image if image is not None else label
    dev = ref.device
    x, y, z = (int(v) for v in ref.shape[:3])
    pr = N.PatchParams()
    for i, (b, p) in enumerate(zip((x, y, z), out_shape)):
        pr.lo[i], pr.before[i], pr.patch[i], pr.flip[i] = 0, b, int(p), 0
    pr.gamma_eps = 1e-7
    c = int(image.shape[3]) if image is not None else 1
    out_image = torch.empty((c,) + tuple(int(p) for p in out_shape), dtype=torch.float32, device=dev) \
        if image is not None else None
    out_label = mask = None
    code = N.LABEL_I64
    if label is not None:
        if label.dtype not in (torch.uint8, torch.int64):
            label = label.to(torch.int64)
        label = label.contiguous()
        code = N.LABEL_U8 if label.dtype == torch.uint8 else N.LABEL_I64
        out_label = torch.empty(tuple(int(p) for p in out_shape), dtype=torch.int64, device=dev)
        mask = torch.empty(1, dtype=torch.int32, device=dev)
        lo_a = (ctypes.c_int32 * 3)(0, 0, 0)
        be_a = (ctypes.c_int32 * 3)(x, y, z)
        N.note_device(dev)
        check(N.lib.ru3d_augment_label_presence(ptr(label), code, x, y, z, lo_a, be_a, 0, ptr(mask), stream()),
              "augment_label_presence")
    ws = N.workspace(N.lib.ru3d_augment_workspace_bytes(*[int(p) for p in out_shape]), dev)
    N.note_device(dev)
    check(N.lib.ru3d_augment_patch(ptr(image), ptr(label), code, x, y, z, c, ctypes.byref(pr), ptr(mask),
                                   ptr(out_image), ptr(out_label), ptr(ws), ws.numel(), stream()), "augment_patch")
    return out_image, out_label


def resample_image(image, out_shape):
    """fp32 device volume [X,Y,Z,C] -> [x,y,z,C] (channels last again), every channel zoomed with order 1."""
    out, _ = _resample(image.to(torch.float32).contiguous(), None, out_shape)
    return out.permute(1, 2, 3, 0).contiguous()


def resample_label(label, out_shape):
    """integer device volume [X,Y,Z] -> int64 [x,y,z] (one-hot / argmax rule for three or more classes)."""
    _, out = _resample(None, label, out_shape)
    return out
