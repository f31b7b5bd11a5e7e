"""Drop-in `data` module: case files, case preparation and its batch drivers (reference data.py).

`CaseDataset`, `load_case`, `save_case`, `save_pred`, `get_spacing`, `apply_scale`, `apply_translate`,
`orient_crop_case`, `batch_load_crop_case`, `resample_normalize_case`, `batch_resample_normalize_case`, `analyze_cases`,
`analyze_raw_cases`, `regions_crop_case`, `batch_regions_crop_case` keep their names, positional arguments and case-dict
layout ({'case_id', 'affine', 'image' float32 [X,Y,Z,C], 'label' int64 [X,Y,Z], 'pred'}).  NIfTI files go through nifti.py
(nibabel when it is installed, a numpy reader / writer of the NIfTI-1 subset the reference uses otherwise); the
affine decomposition restates transforms3d.affines.decompose / compose (a dependency of the reference that is absent
here) for the two helpers that use it.  `orient_crop_case` (data.py:117-172) reorients through this module's
restatement of nibabel's published orientation algebra (`io_orientation`, `apply_orientation`, `inv_ornt_aff`:
nibabel is a dependency of the reference that is absent here, so those three are pinned by their defining property -
every voxel keeps its world coordinate - not by nibabel outputs).

What runs where.  With numpy arrays every function is the reference's arithmetic on the host (numpy / scipy), and no
GPU is needed.  `orient_crop_case`, `resample_normalize_case` and `regions_crop_case` take the device route when the
case holds HIP tensors: reorientation, crop and normalisation are torch data movement on the device, the non-air box,
the zoom and the connected components are HIP kernels (prepare.py, augment.py, components.py), and 'image' / 'label'
come back as HIP tensors.  The batch drivers take one keyword beyond the reference, `device=None`: with a HIP device
each case is uploaded once, prepared through those routes and downloaded to be saved; `analyze_cases` keeps only the
pooled intensity sample in HBM and computes its statistics there.  File reading, gzip and NIfTI parsing stay on the host.

Deliberate departures from the reference: `analyze_cases` keeps one sample list per channel (the reference's
`[[]*n_modality]` is `[[]]` and raises IndexError for a case with two or more channels); `analyze_cases` /
`analyze_raw_cases` take `sample_stride=10` (the reference's fixed `[::10]`).
"""
from pathlib import Path

import numpy as np
import scipy.ndimage as ndi
import torch

import nifti
from transform import crop_pad_to_bbox, remove_small_region, rescale, split_dim  # noqa: F401
from utils import json_load, json_save  # noqa: F401

try:
    from tqdm import tqdm
except Exception:  # pragma: no cover
    def tqdm(x, *a, **k):
        return x


def _case_id(path):
    return str(path).split('/')[-1].split('.')[0]


def _with_channel(image):
    """Cases carry a trailing channel axis; single-modality files are stored as plain 3-D volumes."""
    return image[..., None] if image.ndim == 3 else image


class CaseDataset(torch.utils.data.Dataset):
    """Folder of `<id>.image.nii.gz` (+ `<id>.label.nii.gz`) files -> case dicts (data.py:14-52)."""

    def __init__(self, load_dir, transform=None, load_meta=False):
        super().__init__()
        self.load_dir = Path(load_dir)
        self.transform = transform
        self.image_files = sorted(self.load_dir.glob('*.image.nii.gz'))
        self.label_files = sorted(self.load_dir.glob('*.label.nii.gz'))
        self.load_label = len(self.image_files) == len(self.label_files) and len(self.label_files) > 0

    def __getitem__(self, index):
        case = load_case(self.image_files[index], self.label_files[index] if self.load_label else None)
        return self.transform(case) if self.transform else case

    def __len__(self):
        return len(self.image_files)


class DeviceCaseDataset(torch.utils.data.Dataset):
    """CaseDataset's folder with the cases kept in HBM (not in the reference): a case is loaded and uploaded on first
    access and its augment.DeviceCase kept - with its class-location index built, when max_locations is given -, so

        Trainer(dataset=DeviceCaseDataset(folder, device, max_locations=10000),
                train_transform=DeviceAugment(..., oversample_foreground=0.33),
                dataloader_kwargs={'num_workers': 0})

    uploads and indexes a case once, not once per sample.  Items: {'image': the DeviceCase (DeviceAugment cuts its
    patches from it), 'label': its label tensor, 'case_id': ...}; with a transform, what the transform makes of that."""

    def __init__(self, load_dir, device, max_locations=None, transform=None):
        super().__init__()
        files = CaseDataset(load_dir)
        self.image_files, self.label_files, self.load_label = files.image_files, files.label_files, files.load_label
        self.device, self.max_locations, self.transform = torch.device(device), max_locations, transform
        self.cases = {}

    def __getitem__(self, index):
        index = range(len(self))[index]
        if index not in self.cases:
            from augment import DeviceCase            # augment imports nothing from here; transform imports augment
            case = load_case(self.image_files[index], self.label_files[index] if self.load_label else None)
            resident = DeviceCase(case['image'], case.get('label'), self.device)
            if self.max_locations is not None and resident.label is not None:
                resident.class_index(self.max_locations)
            self.cases[index] = {'image': resident, 'label': resident.label, 'case_id': case['case_id']}
        item = dict(self.cases[index])
        return self.transform(item) if self.transform else item

    def __len__(self):
        return len(self.image_files)


def load_case(image_file, label_file=None):
    image, affine, _ = nifti.load(image_file)
    case = {'case_id': _case_id(image_file), 'affine': affine, 'image': _with_channel(image.astype(np.float32))}
    if label_file:
        label, _, _ = nifti.load(label_file)
        case['label'] = label.astype(np.int64)
    return case


def save_case(case, save_dir):
    save_dir = Path(save_dir)
    save_dir.mkdir(parents=True, exist_ok=True)
    nifti.save(case['image'].astype(np.float32), case['affine'], save_dir / ('%s.image.nii.gz' % case['case_id']))
    for key in ('label', 'pred'):
        if key in case:
            nifti.save(case[key].astype(np.uint8), case['affine'], save_dir / ('%s.%s.nii.gz' % (case['case_id'], key)))


def save_pred(case, save_dir):
    save_dir = Path(save_dir)
    save_dir.mkdir(parents=True, exist_ok=True)
    nifti.save(case['pred'].astype(np.uint8), case['affine'], save_dir / ('%s.pred.nii.gz' % case['case_id']))


# ------------------------------------------------------------------ affine helpers (data.py:55-76)
def get_spacing(affine):
    return tuple(float(np.linalg.norm(affine[i, :3])) for i in range(3))


def _decompose(affine):
    """transforms3d.affines.decompose: A = T . R . diag(Z) . S with S upper-triangular unit shears."""
    a = np.asarray(affine, dtype=np.float64)
    t = a[:3, 3].copy()
    rzs = a[:3, :3]
    zs = np.linalg.cholesky(rzs.T @ rzs).T
    z = np.diag(zs).copy()
    shears = zs / z[:, None]
    r = rzs @ np.linalg.inv(zs)
    if np.linalg.det(r) < 0:
        z[0] *= -1
        zs[0] *= -1
        r = rzs @ np.linalg.inv(zs)
    return t, r, z, shears


def _compose(t, r, z, shears):
    a = np.eye(4)
    a[:3, :3] = r @ np.diag(z) @ shears
    a[:3, 3] = t
    return a


def apply_scale(affine, scale):
    t, r, z, s = _decompose(affine)
    return _compose(t, r, z * np.array(scale), s)


def apply_translate(affine, offset):
    t, r, z, s = _decompose(affine)
    return _compose(t + np.array(offset), r, z, s)


# ------------------------------------------------------------------ orientation (nibabel.orientations, restated)
def io_orientation(affine, tol=None):
    """Orientation of the voxel axes closest to the world axes: [[output axis, +1 | -1 flip], ...] per input axis
    (nibabel.orientations.io_orientation: polar part of the direction cosines by SVD, then a greedy
    largest-component assignment that uses every output axis once)."""
    affine = np.asarray(affine, dtype=np.float64)
    q, p = affine.shape[0] - 1, affine.shape[1] - 1
    rzs = affine[:q, :p]
    zooms = np.sqrt(np.sum(rzs * rzs, axis=0))
    zooms[zooms == 0] = 1
    rs = rzs / zooms
    u, sv, vt = np.linalg.svd(rs, full_matrices=False)
    if tol is None:
        tol = sv.max() * max(rs.shape) * np.finfo(sv.dtype).eps
    keep = sv > tol
    r = np.dot(u[:, keep], vt[keep])
    ornt = np.ones((p, 2), dtype=np.float64) * np.nan
    for in_ax in range(p):
        col = r[:, in_ax]
        if not np.allclose(col, 0):
            out_ax = int(np.argmax(np.abs(col)))
            ornt[in_ax, 0] = out_ax
            ornt[in_ax, 1] = -1 if col[out_ax] < 0 else 1
            r[out_ax, :] = 0          # this output axis is taken
    return ornt


def apply_orientation(arr, ornt):
    """Flip, then permute, the leading axes of `arr` as `ornt` says (nibabel.orientations.apply_orientation)."""
    t = np.asarray(arr)
    ornt = np.asarray(ornt)
    n = ornt.shape[0]
    if t.ndim < n:
        raise ValueError("data array has fewer dimensions than the orientation")
    if np.any(np.isnan(ornt[:, 0])):
        raise ValueError("cannot reorient along a dropped axis")
    for ax, flip in enumerate(ornt[:, 1]):
        if flip == -1:
            t = np.flip(t, axis=ax)
    full = np.arange(t.ndim)
    full[:n] = np.argsort(ornt[:, 0])
    return t.transpose(full)


def inv_ornt_aff(ornt, shape):
    """Affine from the reoriented array's voxel indices back to the original's (nibabel.orientations.inv_ornt_aff)."""
    ornt = np.asarray(ornt)
    p = ornt.shape[0]
    shape = np.array(shape)[:p]
    undo_reorder = np.eye(p + 1)[list(ornt[:, 0].astype(int)) + [p], :]
    undo_flip = np.diag(list(ornt[:, 1]) + [1.0])
    center = -(shape - 1) / 2.0
    undo_flip[:p, p] = ornt[:, 1] * center - center
    return np.dot(undo_flip, undo_reorder)


def reorient(array, affine, ornt):
    """(array, affine) after `ornt` - what nibabel's `Nifti1Pair(array, affine).as_reoriented(ornt)` holds."""
    return apply_orientation(array, ornt), np.dot(np.asarray(affine, dtype=np.float64), inv_ornt_aff(ornt, np.asarray(array).shape))


def _is_hip(x):
    return torch.is_tensor(x) and x.is_cuda


def _apply_orientation_device(t, ornt):
    """apply_orientation for a HIP tensor: flips and a permutation of the leading axes (views; the caller's slice copies)."""
    ornt = np.asarray(ornt)
    n = ornt.shape[0]
    if np.any(np.isnan(ornt[:, 0])):
        raise ValueError("cannot reorient along a dropped axis")
    flips = [ax for ax, flip in enumerate(ornt[:, 1]) if flip == -1]
    if flips:
        t = torch.flip(t, dims=flips)
    full = list(range(t.dim()))
    full[:n] = [int(a) for a in np.argsort(ornt[:, 0])]
    return t.permute(full)


def _orient_crop_case_device(case, air):
    """orient_crop_case for a case whose image is a HIP tensor: the same reorientation and crop as data movement on the
    device, the box from one streaming kernel (prepare.threshold_bbox) instead of np.where's index arrays."""
    import prepare
    case = case.copy()
    device = case['image'].device
    ornt = io_orientation(case['affine'])
    image = case['image']
    new_affine = np.dot(np.asarray(case['affine'], dtype=np.float64), inv_ornt_aff(ornt, tuple(image.shape)))
    image = _apply_orientation_device(image.to(torch.float32), ornt)
    if image.dim() == 3:
        image = image[..., None]
    bbox, _ = prepare.threshold_bbox(image, air)
    box = tuple(slice(int(b[0]), int(b[1])) for b in bbox)
    case['image'] = image[box].contiguous()
    case['bbox'] = bbox
    if 'label' in case:
        label = case['label'] if torch.is_tensor(case['label']) else torch.from_numpy(np.ascontiguousarray(case['label']))
        case['label'] = _apply_orientation_device(label.to(device), ornt)[box].to(torch.int64).contiguous()
    case['affine'] = apply_translate(new_affine, bbox[:, 0] * np.array(get_spacing(new_affine)))
    return case


def orient_crop_case(case, air=-200):
    """data.py:117-172: reorient the case to the closest-to-canonical axes, then crop it to the bounding box of the voxels
    above `air` (in any channel); 'bbox' records the box, the affine moves with the crop.  When `case['image']` is a HIP
    tensor the whole of it runs on the device and 'image' (fp32) / 'label' (int64) come back as HIP tensors, equal to
    the host route's arrays; 'bbox' / 'affine' are numpy either way."""
    if _is_hip(case['image']):
        return _orient_crop_case_device(case, air)
    case = case.copy()
    ornt = io_orientation(case['affine'])
    image, new_affine = reorient(case['image'], case['affine'], ornt)
    image = image.astype(np.float32)
    if 'label' in case:
        label = apply_orientation(case['label'], ornt).astype(np.int64)
    if image.ndim == 3:
        image = image[..., None]
    lo, hi = [], []
    for channel in split_dim(image):
        pos = np.array(np.where(channel > air))
        lo.append(pos.min(axis=1))
        hi.append(pos.max(axis=1))
    bbox = np.array([np.array(lo).min(axis=0), np.array(hi).max(axis=0)]).T          # (3, 2): as in the reference, the
    bbox_c = np.concatenate([bbox, [[0, image.shape[-1]]]])                          # upper bound is the last index itself
    case['image'] = crop_pad_to_bbox(image, bbox_c)
    case['bbox'] = bbox
    if 'label' in case:
        case['label'] = crop_pad_to_bbox(label, bbox)
    case['affine'] = apply_translate(new_affine, bbox[:, 0] * np.array(get_spacing(new_affine)))
    return case


# ------------------------------------------------------------------ preparation (data.py:222-283, 464-492)
def resample_normalize_case(case, target_spacing, normalize_stats):
    """Resample image (and label) to `target_spacing`, clip every channel to its [pct_00_5, pct_99_5] and normalise it
    with (x - mean) / (std + 1e-8).  Host version (scipy zoom); trainer.predict_case runs the same arithmetic on the
    device, and so does this function when `case['image']` is a HIP tensor (augment.resample_image / resample_label)."""
    case = case.copy()
    stats = normalize_stats if isinstance(normalize_stats, list) else [normalize_stats]
    scale = np.array(get_spacing(case['affine'])) / np.array(target_spacing)
    if _is_hip(case['image']):
        import augment
        import inference
        image = case['image'] if case['image'].dim() == 4 else case['image'][..., None]
        shape = inference._zoomed_shape(tuple(int(v) for v in image.shape[:3]), scale)
        case['image'] = inference.resample_normalize_image(image.to(torch.float32).contiguous(), shape, stats)
        if 'label' in case:
            label = case['label'] if torch.is_tensor(case['label']) else torch.from_numpy(np.ascontiguousarray(case['label']))
            case['label'] = augment.resample_label(label.to(image.device), shape)
        case['affine'] = apply_scale(case['affine'], 1 / scale)
        return case
    image = rescale(case['image'], scale, multi_class=True)
    channels = []
    for c, s in enumerate(stats):
        clipped = np.clip(image[..., c], s['pct_00_5'], s['pct_99_5'])
        channels.append((clipped - s['mean']) / (s['std'] + 1e-8))
    case['image'] = np.stack(channels, axis=-1)
    if 'label' in case:
        case['label'] = rescale(case['label'], scale, is_label=True)
    case['affine'] = apply_scale(case['affine'], 1 / scale)
    return case


def regions_crop_case(case, threshold=0, padding=20, based_on='label'):
    """Connected foreground regions of the label (or prediction), each cropped with `padding` millimetres around it.
    When `case[based_on]` is a HIP tensor the boxes come from the device labelling (only the components' sizes and boxes
    cross to the host), and whatever of 'image' / 'label' is a HIP tensor is cropped and padded on the device."""
    if torch.is_tensor(case[based_on]) and case[based_on].is_cuda:
        return _regions_crop_case_device(case, threshold, padding, based_on)
    based = remove_small_region(np.array(case[based_on] > 0), threshold)
    labels, _ = ndi.label(based)
    spacing = np.array(get_spacing(case['affine']))
    pad_vox = np.round(padding / spacing).astype(int)
    regions = []
    for i, sl in enumerate(ndi.find_objects(labels)):
        bbox = np.array([[sl[d].start - pad_vox[d], sl[d].stop + pad_vox[d]] for d in range(3)])
        bbox_c = np.concatenate([bbox, [[0, case['image'].shape[-1]]]])
        region = {'case_id': '%s_%03d' % (case['case_id'], i),
                  'affine': apply_translate(case['affine'], bbox[:, 0] * spacing),
                  'bbox': bbox,
                  'image': crop_pad_to_bbox(case['image'], bbox_c)}
        if 'label' in case:
            region['label'] = crop_pad_to_bbox(case['label'], bbox)
        regions.append(region)
    return regions


def _regions_crop_case_device(case, threshold, padding, based_on):
    import components
    spacing = np.array(get_spacing(case['affine']))
    pad_vox = np.round(padding / spacing).astype(int)

    def crop(volume, bbox):
        if torch.is_tensor(volume) and volume.is_cuda:
            return components.crop_pad_to_bbox(volume, bbox)
        return crop_pad_to_bbox(volume, bbox)

    regions = []
    for i, box in enumerate(components.region_boxes(case[based_on] > 0, threshold)):
        bbox = np.array([[int(box[d][0]) - pad_vox[d], int(box[d][1]) + pad_vox[d]] for d in range(3)])
        bbox_c = np.concatenate([bbox, [[0, case['image'].shape[-1]]]])
        region = {'case_id': '%s_%03d' % (case['case_id'], i),
                  'affine': apply_translate(case['affine'], bbox[:, 0] * spacing),
                  'bbox': bbox,
                  'image': crop(case['image'], bbox_c)}
        if 'label' in case:
            region['label'] = crop(case['label'], bbox)
        regions.append(region)
    return regions


# ------------------------------------------------------------------ batch drivers (data.py:174-220, 287-461, 495-528)
def _files(folder):
    return [path for path in sorted(Path(folder).iterdir()) if path.is_file()]


def _upload(case, device):
    """The case with its volumes as HIP tensors on `device` (labels of 0 .. 255 cross PCIe as bytes)."""
    case = case.copy()
    case['image'] = torch.from_numpy(np.ascontiguousarray(case['image'], dtype=np.float32)).to(device)
    for key in ('label', 'pred'):
        if key in case:
            volume = np.asarray(case[key])
            if volume.size and volume.min() >= 0 and volume.max() <= 255:
                case[key] = torch.from_numpy(np.ascontiguousarray(volume, dtype=np.uint8)).to(device).to(torch.int64)
            else:
                case[key] = torch.from_numpy(np.ascontiguousarray(volume, dtype=np.int64)).to(device)
    return case


def _download(case):
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in case.items()}


def batch_load_crop_case(image_dir, label_dir, save_dir, air=-200, data_range=None, device=None):
    """data.py:174-220: every (image, label) file pair, in sorted order, through orient_crop_case and save_case.
    device: a HIP device runs the reorientation, the non-air box and the crop there (the same volumes, bit for bit)."""
    image_files, label_files = _files(image_dir), _files(label_dir)
    assert len(image_files) == len(label_files), 'number of images is not equal to number of labels.'
    if data_range is None:
        data_range = range(len(image_files))
    for i in tqdm(data_range):
        case = load_case(image_files[i], label_files[i])
        if device is not None:
            case = _download(orient_crop_case(_upload(case, device), air))
        else:
            case = orient_crop_case(case, air)
        save_case(case, save_dir)


def batch_resample_normalize_case(load_dir, save_dir, target_spacing, normalize_stats, data_range=None, device=None):
    """data.py:287-319: every case of `load_dir` through resample_normalize_case and save_case.  device: a HIP device
    runs the zoom (image and label rule) and the normalisation there."""
    cases = CaseDataset(load_dir)
    if data_range is None:
        data_range = range(len(cases))
    for i in tqdm(data_range):
        case = cases[i]
        if device is not None:
            case = _download(resample_normalize_case(_upload(case, device), target_spacing, normalize_stats))
        else:
            case = resample_normalize_case(case, target_spacing, normalize_stats)
        save_case(case, save_dir)


def _intensity_statistics(values):
    """The reference's seven statistics of one pooled sample (data.py:378-388), numpy on the host."""
    return {'median': np.median(values).item(), 'mean': np.mean(values).item(), 'std': np.std(values).item(),
            'min': np.min(values).item(), 'max': np.max(values).item(),
            'pct_00_5': np.percentile(values, 00.5).item(), 'pct_99_5': np.percentile(values, 99.5).item()}


class _HostPool:
    """The pooled sample on the host: the reference's list of arrays, concatenated at the end."""

    def __init__(self):
        self.parts = []

    def append(self, image, label, channel, stride):
        self.parts.append(image[..., channel][np.asarray(label) > 0][::stride])

    def statistics(self):
        return _intensity_statistics(np.concatenate(self.parts))


class _DevicePool:
    """The pooled sample in HBM (prepare.SamplePool) and its statistics from the order-statistics / moments kernels."""

    def __init__(self, device):
        import prepare
        self.prepare = prepare
        self.pool = prepare.SamplePool(device)

    def append(self, image, label, channel, stride):
        self.pool.append(image, label, channel, stride)

    def statistics(self):
        return self.prepare.intensity_statistics(self.pool.values())


def _geometry_props(spacings, shapes):
    spacings, shapes = np.array(spacings), np.array(shapes)
    props = {}
    for name, fn in (('max', np.max), ('min', np.min), ('mean', np.mean), ('median', np.median)):
        props['%s_spacing' % name] = fn(spacings, axis=0).tolist()
        props['%s_shape' % name] = fn(shapes, axis=0).tolist()
    return props


def _merge_props(props_file, new_props):
    if props_file is not None:
        props_file = Path(props_file)
        json_save(str(props_file), {**json_load(str(props_file)), **new_props})
    return new_props


def _analyze(cases, pools, sample_stride, device):
    """Shapes, spacings and the pooled samples of `cases` (an iterable of host case dicts); pools[c] receives channel c
    (a single pool: every channel)."""
    if int(sample_stride) < 1:
        raise ValueError("sample_stride must be >= 1, got %r" % (sample_stride,))
    shapes, spacings = [], []
    for case in cases:
        shapes.append(tuple(int(v) for v in case['image'].shape[:3]))
        spacings.append(get_spacing(case['affine']))
        if device is not None:
            case = _upload(case, device)
        for c in range(case['image'].shape[-1]):
            pools[c if len(pools) > 1 else 0].append(case['image'], case['label'], c, int(sample_stride))
    return _geometry_props(spacings, shapes)


def analyze_cases(load_dir, props_file=None, data_range=None, sample_stride=10, device=None):
    """data.py:322-401: the max / min / mean / median spacing and shape of the cases of `load_dir` and, per channel, the
    statistics of the foreground (label > 0) intensities, every `sample_stride`-th voxel of each case pooled:
    'modality_statstics' (the reference's spelling is the key) is a list of {'median', 'mean', 'std', 'min', 'max',
    'pct_00_5', 'pct_99_5'} - the `normalize_stats` of resample_normalize_case / predict_case.  Returned, and merged
    into `props_file` (existing keys kept) when one is given.
    One list per channel is kept: the reference's `[[]*n_modality]` raises IndexError from the second channel on; for
    one channel the result is the reference's.  sample_stride: 10 is the reference's `[::10]`, 1 takes every foreground
    voxel.  device: a HIP device gathers the samples into one buffer in HBM (prepare.SamplePool) and computes the
    statistics there - order statistics, min and max equal to numpy's, mean and std accumulated in float64."""
    cases = CaseDataset(load_dir)
    n_modality = cases[0]['image'].shape[-1]
    pools = [_DevicePool(device) if device is not None else _HostPool() for _ in range(n_modality)]
    if data_range is None:
        data_range = range(len(cases))
    new_props = _analyze((cases[i] for i in tqdm(data_range)), pools, sample_stride, device)
    new_props['modality_statstics'] = [pool.statistics() for pool in pools]
    return _merge_props(props_file, new_props)


def analyze_raw_cases(image_dir, label_dir, props_file=None, data_range=None, sample_stride=10, device=None):
    """data.py:404-461: analyze_cases on the raw (image, label) file pairs, before any crop.  'modality_statstics' is ONE
    dictionary over the samples of every channel pooled, as in the reference; the shapes are the three spatial extents.
    sample_stride / device: as in analyze_cases."""
    image_files, label_files = _files(image_dir), _files(label_dir)
    assert len(image_files) == len(label_files), 'number of images is not equal to number of labels.'
    pool = _DevicePool(device) if device is not None else _HostPool()
    if data_range is None:
        data_range = range(len(image_files))
    new_props = _analyze((load_case(image_files[i], label_files[i]) for i in tqdm(data_range)), [pool], sample_stride,
                         device)
    new_props['modality_statstics'] = pool.statistics()
    return _merge_props(props_file, new_props)


def batch_regions_crop_case(load_dir, save_dir, threshold=0, padding=20, pred_dir=None, data_range=None, device=None):
    """data.py:495-528: every case of `load_dir` through regions_crop_case, each region saved as a case of its own
    (`<id>_000`, ...).  pred_dir: crop around the components of `<pred_dir>/*.pred.nii.gz` (read as int64 into
    case['pred']) instead of the label's.  device: a HIP device labels the components and crops there."""
    cases = CaseDataset(load_dir)
    pred_files = sorted(Path(pred_dir).glob('*.pred.nii.gz')) if pred_dir is not None else None
    if data_range is None:
        data_range = range(len(pred_files) if pred_dir is not None else len(cases))
    for i in tqdm(data_range):
        case = cases[i]
        if pred_dir is not None:
            case['pred'] = nifti.load(pred_files[i])[0].astype(np.int64)
        if device is not None:
            case = _upload(case, device)
        for region in regions_crop_case(case, threshold, padding, 'pred' if pred_dir is not None else 'label'):
            save_case(_download(region), save_dir)
