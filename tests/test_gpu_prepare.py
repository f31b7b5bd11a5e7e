"""Dataset preparation on the HIP path (csrc/prepare.hip, prepare.py, the device routes of data.py) against numpy and
against the host routes of the same functions.  The non-air box, the crop, the masked sample and every order statistic
are compared with `==`; mean and standard deviation against numpy on the samples cast to float64 (1e-10 relative) and
against the host route's float32 values (1e-5); the zoom by the yardsticks test_gpu_augment.py / test_gpu_predict.py
apply to the same kernel.  `-m gpu` only."""
import gzip

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no HIP device", allow_module_level=True)

import _native as N  # noqa: E402
import data  # noqa: E402
import nifti  # noqa: E402
import prepare  # noqa: E402

DEV = torch.device("cuda:0")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np_box(img, thr):
    pos = np.array(np.where((img > thr).any(axis=-1)))
    return np.array([pos.min(axis=1), pos.max(axis=1)]).T, pos.shape[1]


# ------------------------------------------------------------------------------------------------ box
@pytest.mark.parametrize("shape", [(37, 41, 67, 2), (9, 7, 3, 1), (16, 16, 16, 4), (5, 6, 7, 3), (4, 3, 5, 5), (40, 33, 50, 1)])
def test_threshold_bbox_is_np_where(shape):
    rng = np.random.RandomState(sum(shape))
    img = np.full(shape, -1000.0, dtype=np.float32)
    x0, y0, z0 = shape[0] // 4, shape[1] // 3, shape[2] // 5
    img[x0:x0 + shape[0] // 2 + 1, y0:y0 + shape[1] // 2 + 1, z0:z0 + shape[2] // 2 + 1] = \
        rng.rand(shape[0] // 2 + 1, shape[1] // 2 + 1, shape[2] // 2 + 1, shape[3]).astype(np.float32) * 600 - 300
    want, count = _np_box(img, -200)
    got, n = prepare.threshold_bbox(_dev(img), -200)
    assert np.array_equal(got, want) and n == count
    view = _dev(np.concatenate([img, img], axis=0))[1:shape[0] + 1]      # a slice: made contiguous by the wrapper
    got, n = prepare.threshold_bbox(view, -200)
    assert np.array_equal(got, _np_box(np.concatenate([img, img], axis=0)[1:shape[0] + 1], -200)[0])


def test_threshold_bbox_corner_cases():
    img = np.full((11, 13, 17, 2), -1000.0, dtype=np.float32)
    with pytest.raises(ValueError):
        prepare.threshold_bbox(_dev(img), -200)                          # nothing above: numpy's min of an empty array
    one = img.copy()
    one[10, 0, 16, 1] = 5.0                                              # a single voxel, decided by the second channel
    got, n = prepare.threshold_bbox(_dev(one), -200)
    assert np.array_equal(got, [[10, 10], [0, 0], [16, 16]]) and n == 1
    faces = img.copy()
    faces[0, 5, 5, 0] = faces[10, 5, 5, 0] = faces[4, 0, 3, 1] = faces[4, 12, 3, 0] = faces[4, 4, 0, 1] = faces[4, 4, 16, 0] = 1.0
    got, n = prepare.threshold_bbox(_dev(faces), -200)
    assert np.array_equal(got, [[0, 10], [0, 12], [0, 16]]) and n == 6
    with pytest.raises(ValueError):
        prepare.threshold_bbox(_dev(faces), 1.0)                         # strictly above
    full = np.zeros((6, 5, 9), dtype=np.float32)                         # a 3-D volume, every voxel above
    got, n = prepare.threshold_bbox(_dev(full), -200)
    assert np.array_equal(got, [[0, 5], [0, 4], [0, 8]]) and n == full.size
    img[3, 3, 3, 0] = np.nan                                             # NaN compares false, as in numpy
    with pytest.raises(ValueError):
        prepare.threshold_bbox(_dev(img), -200)


# ------------------------------------------------------------------------------------------------ masked sample
@pytest.mark.parametrize("dtype", [np.uint8, np.int64])
@pytest.mark.parametrize("stride", [1, 7, 10])
def test_masked_sample_is_numpy_fancy_indexing(dtype, stride):
    rng = np.random.RandomState(stride)
    for shape in [(37, 41, 67, 2), (5, 3, 2, 1), (33, 64, 65, 1)]:
        img = rng.randn(*shape).astype(np.float32)
        lab = (rng.rand(*shape[:3]) < 0.3).astype(dtype) * rng.randint(1, 4, size=shape[:3]).astype(dtype)
        if dtype == np.int64:
            lab[rng.rand(*shape[:3]) < 0.05] = -3                        # `label > 0` is a signed comparison
        for c in range(shape[3]):
            want = img[..., c][lab > 0][::stride]
            got = prepare.masked_sample(_dev(img), _dev(lab), c, stride)
            assert got.dtype == torch.float32 and np.array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize("stride", [1, 7])
def test_masked_sample_scans_more_than_1024_chunk_counts(stride):
    """(129, 128, 128): 1032 chunks of 2048 voxels, so the one-workgroup scan of the chunk counts gives a thread two
    chunks and the chunk count is no multiple of its 1024 threads."""
    rng = np.random.RandomState(stride)
    shape = (129, 128, 128, 1)
    img = rng.randn(*shape).astype(np.float32)
    lab = (rng.rand(*shape[:3]) < 0.3).astype(np.uint8)
    got = prepare.masked_sample(_dev(img), _dev(lab), 0, stride)
    assert got.dtype == torch.float32 and np.array_equal(got.cpu().numpy(), img[..., 0][lab > 0][::stride])


def test_masked_sample_counts_and_buffers():
    rng = np.random.RandomState(0)
    img = rng.randn(20, 21, 23, 1).astype(np.float32)
    d_img = _dev(img)
    empty = np.zeros((20, 21, 23), dtype=np.uint8)
    assert prepare.masked_sample(d_img, _dev(empty), 0, 10).numel() == 0
    full = np.ones((20, 21, 23), dtype=np.uint8)
    assert np.array_equal(prepare.masked_sample(d_img, _dev(full), 0, 1).cpu().numpy(), img.reshape(-1))
    assert np.array_equal(prepare.masked_sample(d_img, _dev(full), 0, 7).cpu().numpy(), img.reshape(-1)[::7])
    lab = np.zeros(20 * 21 * 23, dtype=np.uint8)
    lab[rng.permutation(lab.size)[:700]] = 1                              # 700 = 70 * 10: an exact multiple of the stride
    lab = lab.reshape(20, 21, 23)
    assert prepare.masked_sample(d_img, _dev(lab), 0, 10).numel() == 70
    lab.reshape(-1)[np.flatnonzero(lab.reshape(-1) == 0)[0]] = 1          # 701: one more sample
    assert prepare.masked_sample(d_img, _dev(lab), 0, 10).numel() == 71
    want = img[..., 0][lab > 0][::10]
    pool = torch.full((200,), -7.0, dtype=torch.float32, device=DEV)      # appended at an offset of a shared buffer
    view = prepare.masked_sample(d_img, _dev(lab), 0, 10, out=pool[50:50 + 71])
    assert view.numel() == 71 and view.data_ptr() == pool[50:].data_ptr()
    host = pool.cpu().numpy()
    assert np.array_equal(host[50:121], want) and (host[:50] == -7).all() and (host[121:] == -7).all()
    pool.fill_(-7.0)
    with pytest.raises(ValueError):
        prepare.masked_sample(d_img, _dev(lab), 0, 10, out=pool[50:50 + 60])   # too small: an error ...
    host = pool.cpu().numpy()
    assert (host[:50] == -7).all() and (host[110:] == -7).all()          # ... and nothing written past the buffer
    sp = prepare.SamplePool(DEV, capacity=16)                             # grows geometrically, keeps what it holds
    assert sp.append(d_img, _dev(lab), 0, 10) == 71 and sp.append(d_img, _dev(full), 0, 7) == len(img.reshape(-1)[::7])
    assert np.array_equal(sp.values().cpu().numpy(), np.concatenate([want, img.reshape(-1)[::7]]))


# ------------------------------------------------------------------------------------------------ order statistics
def _check_order(values, ranks):
    got = prepare.order_statistics(_dev(values), ranks)
    want = np.sort(values)[list(ranks)]
    assert got.dtype == np.float32 and (got == want).all(), (got, want)


def test_order_statistics_are_np_sort():
    rng = np.random.RandomState(1)
    _check_order(np.array([3.5], dtype=np.float32), [0])
    _check_order(np.array([2.0, -1.0], dtype=np.float32), [0, 1])
    v = (rng.randn(1000) * 50).astype(np.float32)
    _check_order(v, [0, 1, 499, 500, 998, 999])
    ranks = [0, 4, 5, 500, 994, 995, 997, 998]                           # eight ranks, a buffer that is not 16-byte aligned
    assert (prepare.order_statistics(_dev(v)[1:], ranks) == np.sort(v[1:])[ranks]).all()
    dup = np.repeat(np.array([-3.0, 0.0, -0.0, 7.0, 7.0, 1e-30, -1e-30], dtype=np.float32), 300)
    rng.shuffle(dup)
    _check_order(dup, [0, 299, 300, 900, 1199, 1500, 2099])
    base = np.float32(1.0)
    near = np.array([base, np.nextafter(base, np.float32(2)), np.nextafter(base, np.float32(0))] * 111, dtype=np.float32)
    _check_order(near, [0, 110, 111, 221, 222, 332])                     # values one mantissa bit apart
    big = np.round(rng.randn(5_000_003) * 120 + 80).astype(np.float32)   # integer-valued, CT-like, long runs of equal values
    big[::1000] = rng.randn(len(big[::1000])).astype(np.float32) * 1e4
    n = big.size
    _check_order(big, [0, 1, n // 200, n // 2 - 1, n // 2, n - n // 200, n - 2, n - 1])
    with pytest.raises(ValueError):
        prepare.order_statistics(_dev(v), [1000])
    with pytest.raises(ValueError):
        prepare.order_statistics(_dev(v), list(range(9)))


def _check_statistics(values, exact_quantiles):
    got = prepare.intensity_statistics(_dev(values))
    assert list(got) == ['median', 'mean', 'std', 'min', 'max', 'pct_00_5', 'pct_99_5']
    assert all(type(v) is float for v in got.values())
    assert got['min'] == values.min().item() and got['max'] == values.max().item()
    want = {'median': np.median(values), 'pct_00_5': np.percentile(values, 0.5), 'pct_99_5': np.percentile(values, 99.5)}
    for key, w in want.items():
        if exact_quantiles:
            assert got[key] == w.item(), key
        else:
            assert abs(np.float32(got[key]) - w) <= np.spacing(np.abs(w)), key
    v64 = values.astype(np.float64)
    assert abs(got['mean'] - v64.mean()) <= 1e-10 * abs(v64.mean()) + 1e-300
    assert abs(got['std'] - v64.std()) <= 1e-10 * v64.std()
    assert abs(got['mean'] - values.mean().item()) <= 1e-5 * abs(values.mean().item())
    assert abs(got['std'] - values.std().item()) <= 1e-5 * values.std().item()
    assert prepare.intensity_statistics(_dev(values)) == got               # the same bits from run to run
    return got


def test_intensity_statistics_against_numpy():
    rng = np.random.RandomState(2)
    ct = np.round(rng.randn(300_001) * 80 + 100).astype(np.float32)
    _check_statistics(ct, exact_quantiles=True)
    _check_statistics(ct[:300_000], exact_quantiles=True)
    _check_statistics((rng.randn(200_003) * 3 + 1).astype(np.float32), exact_quantiles=False)
    with pytest.raises(ValueError):
        prepare.intensity_statistics(_dev(np.array([1.0, np.nan], dtype=np.float32)))


def test_streaming_passes_with_a_capped_grid():
    """The streaming grids (box, radix-select passes, both moment passes) are capped at 8 blocks a CU of the budget, four
    values a thread and trip.  The box of (37, 41, 67, 2): 101639 voxels = 100 blocks of 256 threads uncapped; the
    statistics of 300001 values: 293 blocks - both under the 2048 of the whole chip, both over the 64 of a budget of 8 CUs,
    where the loops make a second trip and more.  The comparisons are test_threshold_bbox_is_np_where's and
    test_intensity_statistics_against_numpy's."""
    rng = np.random.RandomState(3)
    img = np.full((37, 41, 67, 2), -1000.0, dtype=np.float32)
    img[9:28, 13:34, 13:47] = rng.rand(19, 21, 34, 2).astype(np.float32) * 600 - 300
    img[36, 40, 66, 1] = 0.0                                              # the last voxel: the last trip of the last block
    want, count = _np_box(img, -200)
    ct = np.round(rng.randn(300_001) * 80 + 100).astype(np.float32)
    full = prepare.intensity_statistics(_dev(ct))
    try:
        assert N.lib.ru3d_set_cu_budget(8) == 0
        got, n = prepare.threshold_bbox(_dev(img), -200)
        stats = _check_statistics(ct, exact_quantiles=True)
    finally:
        N.lib.ru3d_set_cu_budget(0)
    assert N.lib.ru3d_get_cu_budget() == torch.cuda.get_device_properties(DEV).multi_processor_count
    assert np.array_equal(got, want) and n == count
    for key in ('median', 'min', 'max', 'pct_00_5', 'pct_99_5'):           # selected values: the same whatever the grid
        assert stats[key] == full[key], key


# ------------------------------------------------------------------------------------------------ data.py, case by case
def _flipped_case(channels=1):
    rng = np.random.RandomState(3)
    vol = np.full((12, 10, 9) + ((channels,) if channels > 1 else ()), -1000.0, dtype=np.float32)
    vol[3:8, 2:7, 4:8] = rng.rand(*((5, 5, 4) + vol.shape[3:])).astype(np.float32) * 100
    label = ((vol if channels == 1 else vol[..., 0]) > 50).astype(np.int64) * 2
    aff = np.array([[0, -1.5, 0, 10.0], [2.0, 0, 0, -4.0], [0, 0, -3.0, 7.0], [0, 0, 0, 1.0]])   # axes swapped, two flipped
    return {"case_id": "c", "image": vol, "label": label, "affine": aff}


@pytest.mark.parametrize("channels", [1, 2])
def test_orient_crop_case_on_the_device_is_the_host_route(channels):
    case = _flipped_case(channels)
    want = data.orient_crop_case(case, air=-200)
    got = data.orient_crop_case({**case, "image": _dev(case["image"]), "label": _dev(case["label"])}, air=-200)
    assert got["image"].is_cuda and got["image"].dtype == torch.float32 and got["image"].is_contiguous()
    assert got["label"].is_cuda and got["label"].dtype == torch.int64
    assert np.array_equal(got["image"].cpu().numpy(), want["image"]) and want["image"].size > 0
    assert np.array_equal(got["label"].cpu().numpy(), want["label"])
    assert isinstance(got["bbox"], np.ndarray) and np.array_equal(got["bbox"], want["bbox"])
    assert isinstance(got["affine"], np.ndarray) and np.array_equal(got["affine"], want["affine"])
    assert not torch.is_tensor(case["image"])                             # the caller's case is left alone


def _blob_case(num_classes, shape=(40, 36, 30), seed=4):
    rng = np.random.RandomState(seed)
    g = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing="ij"), axis=-1).astype(np.float64)
    r = np.sqrt((((g - np.array(shape) / 2.0) / (np.array(shape) / 2.6)) ** 2).sum(axis=-1))
    image = np.where(r < 1, 60 + 200 * (1 - r), -1000).astype(np.float32) + rng.randn(*shape).astype(np.float32) * 5
    label = np.zeros(shape, dtype=np.int64)
    label[r < 0.55] = 1
    if num_classes > 2:
        label[r < 0.3] = 2
    aff = np.diag([1.2, 1.5, 2.5, 1.0])
    aff[:3, 3] = [-20.0, 11.0, 5.0]
    return {"case_id": "blob%d" % num_classes, "image": image[..., None], "label": label, "affine": aff}


STATS = {"mean": 100.25, "std": 76.5, "pct_00_5": -79.0, "pct_99_5": 303.0}


@pytest.mark.parametrize("num_classes", [2, 3])
def test_resample_normalize_case_on_the_device_is_the_host_route(num_classes):
    case = _blob_case(num_classes)
    target = (1.0, 1.3, 1.9)
    want = data.resample_normalize_case(case, target, STATS)
    got = data.resample_normalize_case({**case, "image": _dev(case["image"]), "label": _dev(case["label"])}, target, STATS)
    assert got["image"].is_cuda and tuple(got["image"].shape) == want["image"].shape
    assert np.array_equal(got["affine"], want["affine"])
    # the zoom kernel against scipy: test_gpu_augment.py holds it to 2e-6 on unit-range data; here the clipped range is
    # 382 wide before the division by the standard deviation
    assert np.abs(got["image"].cpu().numpy() - want["image"]).max() < 2e-5
    lab = got["label"].cpu().numpy()
    assert got["label"].dtype == torch.int64 and lab.shape == want["label"].shape
    assert (lab != want["label"]).mean() < 2e-3                           # ties of the interpolated one-hot maps only
    assert set(np.unique(lab)) == set(range(num_classes))


# ------------------------------------------------------------------------------------------------ data.py, the drivers
def _write_raw(folder):
    images, labels = folder / "imagesTr", folder / "labelsTr"
    images.mkdir(parents=True), labels.mkdir(parents=True)
    for i, case in enumerate([_blob_case(2, (40, 36, 30), 5), _blob_case(3, (34, 38, 28), 6), _blob_case(3, (36, 30, 32), 7)]):
        image, label, aff = case["image"][..., 0], case["label"], case["affine"]
        if i == 0:                                                        # stored with swapped and flipped axes
            image, label = image.transpose(1, 0, 2)[::-1], label.transpose(1, 0, 2)[::-1]
            aff = np.array([[0, 1.2, 0, -20.0], [-1.5, 0, 0, 60.0], [0, 0, 2.5, 5.0], [0, 0, 0, 1.0]])
        nifti.save(np.ascontiguousarray(image), aff, images / ("case_%02d.nii.gz" % i))
        nifti.save(np.ascontiguousarray(label).astype(np.uint8), aff, labels / ("case_%02d.nii.gz" % i))
    return images, labels


def _same_files(a, b):
    names = sorted(p.name for p in a.iterdir())
    assert names and names == sorted(p.name for p in b.iterdir())
    for name in names:                                                    # the gzip header carries a time stamp
        assert gzip.decompress((a / name).read_bytes()) == gzip.decompress((b / name).read_bytes()), name
    return names


def test_batch_drivers_on_the_device_against_the_host(tmp_path):
    images, labels = _write_raw(tmp_path / "raw")
    host, dev = tmp_path / "host", tmp_path / "dev"
    data.batch_load_crop_case(images, labels, host / "crop", -200)
    data.batch_load_crop_case(images, labels, dev / "crop", -200, device="cuda:0")
    assert len(_same_files(host / "crop", dev / "crop")) == 6

    for stride in (10, 1):
        want = data.analyze_cases(host / "crop", sample_stride=stride)
        got = data.analyze_cases(dev / "crop", sample_stride=stride, device="cuda:0")
        assert {k: v for k, v in got.items() if k != "modality_statstics"} == \
            {k: v for k, v in want.items() if k != "modality_statstics"}
        (w,), (g,) = want["modality_statstics"], got["modality_statstics"]
        for key in ("min", "max"):
            assert g[key] == w[key]
        for key in ("median", "pct_00_5", "pct_99_5"):
            assert abs(np.float32(g[key]) - np.float32(w[key])) <= np.spacing(np.abs(np.float32(w[key]))), key
        for key in ("mean", "std"):
            assert abs(g[key] - w[key]) <= 1e-5 * abs(w[key]), key
    raw_w = data.analyze_raw_cases(images, labels)
    raw_g = data.analyze_raw_cases(images, labels, device="cuda:0")
    assert isinstance(raw_g["modality_statstics"], dict) and raw_g["max_shape"] == raw_w["max_shape"]
    assert raw_g["modality_statstics"]["min"] == raw_w["modality_statstics"]["min"]
    assert abs(raw_g["modality_statstics"]["std"] - raw_w["modality_statstics"]["std"]) <= 1e-5 * raw_w["modality_statstics"]["std"]

    data.batch_regions_crop_case(host / "crop", host / "region", threshold=50, padding=4)
    data.batch_regions_crop_case(dev / "crop", dev / "region", threshold=50, padding=4, device="cuda:0")
    assert len(_same_files(host / "region", dev / "region")) == 6
    for name in ("host", "dev"):                                          # the label doubles as a prediction
        (tmp_path / name / "pred").mkdir()
        for f in sorted((tmp_path / name / "crop").glob("*.label.nii.gz")):
            vol, aff, _ = nifti.load(f)
            nifti.save(vol.astype(np.uint8), aff, tmp_path / name / "pred" / f.name.replace(".label.", ".pred."))
    data.batch_regions_crop_case(host / "crop", host / "region_p", 50, 4, host / "pred", range(2))
    data.batch_regions_crop_case(dev / "crop", dev / "region_p", 50, 4, dev / "pred", range(2), device="cuda:0")
    assert len(_same_files(host / "region_p", dev / "region_p")) == 4

    stats = want["modality_statstics"]
    target = (1.0, 1.3, 1.9)
    data.batch_resample_normalize_case(host / "crop", host / "norm", target, stats)
    data.batch_resample_normalize_case(dev / "crop", dev / "norm", target, stats, device="cuda:0")
    names = sorted(p.name for p in (host / "norm").iterdir())
    assert len(names) == 6 and names == sorted(p.name for p in (dev / "norm").iterdir())
    for name in names:
        a, aff_a, _ = nifti.load(host / "norm" / name)
        b, aff_b, _ = nifti.load(dev / "norm" / name)
        assert a.shape == b.shape and np.array_equal(aff_a, aff_b)
        if ".image." in name:
            assert np.abs(a - b).max() < 2e-5, name
        else:
            assert (a != b).mean() < 2e-3, name
