"""Foreground oversampling on the device: the class-location index (csrc/locations.hip behind ru3d_class_index) against its
numpy twin `transform.class_locations`, exactly; the sampler with oversample_foreground against the numpy crops under one
seed (labels identical, images within 2e-5 - the tolerances of test_gpu_augment.py for this pipeline); no transfer to
the host on a forced patch; `data.DeviceCaseDataset`.  A tile is 2048 voxels (PP_CHUNK), a scan thread owns more than one
tile count from 1025 tiles on (BV_SCAN_THREADS = 1024).  Run with `-m gpu`."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no HIP device", allow_module_level=True)

import augment  # noqa: E402
import data  # noqa: E402
import transform as T  # noqa: E402

DEV = torch.device("cuda:0")
TILE = 2048


# ------------------------------------------------------------------------------------------------ the index
def _blobs(shape, seed):
    """Spatially coherent classes 0 .. 3 with a sprinkle of single voxels of 4 .. 9."""
    rng = np.random.RandomState(seed)
    g = np.meshgrid(*[np.linspace(-1, 1, s, dtype=np.float32) for s in shape], indexing="ij")
    lab = np.zeros(shape, dtype=np.uint8)
    lab[np.sqrt(g[0] ** 2 + (1.2 * g[1]) ** 2 + g[2] ** 2) < 0.8] = 1
    lab[np.sqrt((g[0] - 0.2) ** 2 + g[1] ** 2 + g[2] ** 2) < 0.35] = 2
    lab[np.sqrt((g[0] + 0.3) ** 2 + (g[1] - 0.1) ** 2 + g[2] ** 2) < 0.2] = 3
    flat = lab.reshape(-1)
    where = rng.randint(0, flat.size, size=60)
    flat[where] = rng.randint(4, 10, size=60)
    return lab


def _volume(name):
    rng = np.random.RandomState(len(name))
    if name == "below_one_trip":                                   # 210 voxels: less than a workgroup trip of 256
        return rng.randint(0, 4, size=(5, 6, 7))
    if name == "one_tile":
        return rng.randint(0, 5, size=(16, 16, 8))
    if name == "one_tile_and_a_voxel":
        lab = rng.randint(0, 3, size=(1, 3, 683))
        assert lab.size == TILE + 1
        lab[0, 2, 682] = 9                                         # the one voxel of the second tile, alone in its class
        return lab
    if name == "partial_last_tile":
        lab = rng.randint(0, 4, size=(33, 17, 13))
        assert lab.size > 3 * TILE and lab.size % TILE
        lab.reshape(-1)[3 * TILE + 700::37] = 5                    # a class that lives in the last, partial tile only
        return lab
    if name == "all_32_classes_in_every_wave":
        return rng.randint(0, 32, size=(33, 17, 13))
    if name == "one_class":
        return np.full((16, 16, 9), 4)
    if name == "air":
        return np.zeros((9, 16, 16), dtype=np.int64)
    if name == "runs_across_waves_and_tiles":
        return ((np.arange(20 * 20 * 20) // 100) % 4).reshape(20, 20, 20)
    if name == "values_outside":
        lab = rng.randint(0, 3, size=(12, 11, 20)).astype(np.int64)
        lab.reshape(-1)[::7] = -3
        lab.reshape(-1)[3::11] = 40
        lab.reshape(-1)[5::13] = 31
        return lab
    if name == "more_tiles_than_scan_threads":
        lab = _blobs((160, 128, 112), 5)
        assert lab.size // TILE > 1024
        return lab
    raise KeyError(name)


def _expected(label, m):
    counts, boxes, rows = T.class_locations(label, m)
    table = np.full((32, m), -1, dtype=np.int32)
    for c, row in enumerate(rows):
        table[c, :len(row)] = row
    return counts, boxes, rows, table


def _hold_index(label, dtype, m):
    label = np.ascontiguousarray(label.astype(dtype))
    index = augment.ClassIndex(torch.from_numpy(label).to(DEV), m)
    counts, boxes, rows, table = _expected(label, m)
    assert index.counts.dtype == np.int64 and np.array_equal(index.counts, counts)
    assert index.boxes.dtype == np.int32 and np.array_equal(index.boxes, boxes)
    got = index.device_locations
    assert got.dtype == torch.int32 and tuple(got.shape) == (32, m)
    assert np.array_equal(got.cpu().numpy(), table)                # every row, the -1 padding included
    assert index.classes() == [c for c in range(1, 32) if counts[c] > 0]
    for c in (0, 1, 5, 31):
        assert np.array_equal(index.locations(c), rows[c]) and index.locations(c).dtype == np.int32
    return index


SMALL = ["below_one_trip", "one_tile", "one_tile_and_a_voxel", "partial_last_tile", "all_32_classes_in_every_wave", "one_class",
         "air", "runs_across_waves_and_tiles"]


@pytest.mark.parametrize("m", [1, 7, 10000])
@pytest.mark.parametrize("dtype", [np.uint8, np.int64])
@pytest.mark.parametrize("name", SMALL)
def test_index_equals_the_numpy_twin(name, dtype, m):
    _hold_index(_volume(name), dtype, m)


@pytest.mark.parametrize("m", [1, 7, 10000])
def test_index_ignores_negative_and_large_int64_values(m):
    index = _hold_index(_volume("values_outside"), np.int64, m)
    assert index.counts.sum() < 12 * 11 * 20 and index.counts[31] > 0


@pytest.mark.parametrize("dtype,m", [(np.uint8, 10000), (np.int64, 7), (np.uint8, 1)])
def test_index_of_more_tiles_than_scan_threads(dtype, m):
    index = _hold_index(_volume("more_tiles_than_scan_threads"), dtype, m)
    assert index.counts[0] > 10000 and index.counts[1] > 10000     # strided rows and complete ones in one build
    assert 0 < index.counts[3] < 10000


def test_two_builds_are_the_same_bits():
    label = torch.from_numpy(_volume("more_tiles_than_scan_threads")).to(DEV)
    a, b = augment.ClassIndex(label, 500), augment.ClassIndex(label, 500)
    assert torch.equal(a.device_locations, b.device_locations)
    assert np.array_equal(a.counts, b.counts) and np.array_equal(a.boxes, b.boxes)
    noisy = torch.from_numpy(_volume("all_32_classes_in_every_wave").astype(np.uint8)).to(DEV)
    assert torch.equal(augment.ClassIndex(noisy, 64).device_locations, augment.ClassIndex(noisy, 64).device_locations)


def test_the_case_keeps_its_index():
    label = _volume("partial_last_tile").astype(np.uint8)
    case = augment.DeviceCase(np.zeros(label.shape + (1,), np.float32), label, DEV)
    first = case.class_index()
    assert first.max_per_class == 10000 and case.class_index() is first and case.class_index(10000) is first
    other = case.class_index(7)
    assert other is not first and other.max_per_class == 7 and case.class_index(7) is other
    assert len(other.locations(1)) == 7 and other.device_locations.is_cuda
    with pytest.raises(ValueError):
        augment.DeviceCase(np.zeros((4, 4, 4, 1), np.float32), None, DEV).class_index()
    with pytest.raises(ValueError):
        case.class_index(0)


# ------------------------------------------------------------------------------------------------ the sampler
SHAPE, PATCH = (96, 80, 72), (64, 64, 64)
SPATIAL = dict(rotation=((-0.3, 0.3), (-0.1, 0.1), (0, 0.2)), elastic_spacing=16, elastic_magnitude=(0, 4))
INTENSITY = (("contrast", T.adjust_contrast), ("brightness", T.adjust_brightness), ("gamma", T.adjust_gamma))


def _four_classes(shape=SHAPE, seed=0):
    rng = np.random.RandomState(seed)
    g = np.meshgrid(*[np.linspace(-1, 1, s, dtype=np.float32) for s in shape], indexing="ij")
    img = (np.sin(4 * g[0]) * np.cos(3 * g[1]) + g[2] ** 2 + 0.05 * rng.randn(*shape)).astype(np.float32)[..., None]
    lab = np.zeros(shape, dtype=np.uint8)
    lab[np.sqrt(g[0] ** 2 + (1.2 * g[1]) ** 2 + g[2] ** 2) < 0.8] = 1
    lab[np.sqrt((g[0] - 0.2) ** 2 + g[1] ** 2 + g[2] ** 2) < 0.35] = 2
    lab[np.sqrt((g[0] + 0.6) ** 2 + (g[1] - 0.5) ** 2 + (g[2] + 0.5) ** 2) < 0.12] = 3      # small, off centre
    return img, lab


@pytest.fixture(scope="module")
def volume():
    img, lab = _four_classes()
    case = augment.DeviceCase(img, lab, DEV)
    img.setflags(write=False), lab.setflags(write=False)          # shared by the tests below: read only
    return img, lab, case


def _twin_patches(img, lab, seed, count, spatial, **kw):
    """`count` consecutive patches of the numpy chain under one seed: crop -> RandomMirror -> contrast, brightness, gamma
    (DeviceAugment's defaults: p = 0.5 per axis, factors in [0.9, 1.1])."""
    crop = T.RandomSpatialCrop(0.1, list(PATCH), crop_mode="random", **SPATIAL, **kw) if spatial else \
        T.RandomRescaleCrop(0.1, list(PATCH), crop_mode="random", **kw)
    np.random.seed(seed)
    out = []
    for _ in range(count):
        case = crop({"image": img.copy(), "label": lab.copy()})
        image, label = case["image"], case["label"]
        for axis in range(3):
            if np.random.uniform() < 0.5:
                image, label = np.flip(image, axis).copy(), np.flip(label, axis).copy()
        for _, op in INTENSITY:
            image = op(image, np.random.uniform(0.9, 1.1))
        out.append((np.moveaxis(image, -1, 0), label.astype(np.int64)))
    return out


@pytest.mark.parametrize("spatial", [False, True], ids=["plain", "rotation_elastic"])
@pytest.mark.parametrize("kw", [dict(oversample_foreground=0.5), dict(oversample_foreground=1.0, foreground_classes=[3])],
                         ids=["p_0.5_all_classes", "p_1_class_3"])
def test_same_seed_same_patch_as_the_numpy_twin(volume, kw, spatial):
    img, lab, case = volume
    count = 10                                                     # forced and unforced draws interleave under one seed
    want = _twin_patches(img, lab, 31, count, spatial, **kw)
    aug = augment.DeviceAugment(scale=0.1, crop_size=list(PATCH), crop_mode="random", **(SPATIAL if spatial else {}), **kw)
    np.random.seed(31)
    got = [aug.sample(case) for _ in range(count)]
    torch.cuda.synchronize()
    with_3 = 0
    for i, ((got_img, got_lab), (want_img, want_lab)) in enumerate(zip(got, want)):
        differ = int((got_lab.cpu().numpy() != want_lab).sum())
        err = float(np.abs(got_img.cpu().numpy() - want_img).max())
        print("patch %d: %d label voxels differ, max |image difference| %.3g" % (i, differ, err))
        assert differ == 0, i
        assert err <= 2e-5, i
        with_3 += int((want_lab == 3).any())
    if "foreground_classes" in kw and not spatial:
        assert with_3 == count                                     # the axis-aligned box holds its voxel


def test_the_presence_mask_of_a_forced_patch_has_the_bit_of_its_class(volume):
    _, _, case = volume
    aug = augment.DeviceAugment(scale=0.1, crop_size=32, crop_mode="random", oversample_foreground=1.0, foreground_classes=[3])
    np.random.seed(2)
    for _ in range(8):
        drawn = aug._draw(case)
        _, label = aug._launch(case, drawn, None, None, None)
        torch.cuda.synchronize()
        assert (int(drawn[1].item()) >> 3) & 1                     # read after the call: no readback inside it
        assert bool((label == 3).any())


def test_a_forced_patch_reads_nothing_back(volume, monkeypatch):
    img, lab, _ = volume
    case = augment.DeviceCase(img.copy(), lab.copy(), DEV)         # a case of its own: its index is built below
    aug = augment.DeviceAugment(scale=0.1, crop_size=32, crop_mode="random", oversample_foreground=1.0)
    enforce = augment.DeviceAugment(scale=0.1, crop_size=32, crop_mode="random", enforce_label_indices=[1])
    np.random.seed(4)
    aug.sample(case)                                               # the first patch of the case builds its index
    enforce.sample(case)

    def refuse(*a, **k):
        raise AssertionError("a transfer to the host")

    for name in ("item", "cpu", "tolist", "numpy"):
        monkeypatch.setattr(torch.Tensor, name, refuse)
    patches = [aug.sample(case) for _ in range(4)]
    with pytest.raises(AssertionError, match="a transfer to the host"):
        enforce.sample(case)                                       # the check bites: this route reads its mask back
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert all(int((lab_ > 0).sum()) > 0 for _, lab_ in patches)


def test_defaults_are_the_sampler_without_the_keywords(volume):
    _, _, case = volume
    for extra in ({}, SPATIAL):
        np.random.seed(8)
        want = [augment.DeviceAugment(scale=0.1, crop_size=48, **extra).sample(case) for _ in range(3)]
        np.random.seed(8)
        got = [augment.DeviceAugment(scale=0.1, crop_size=48, oversample_foreground=None, foreground_classes=None,
                                     max_locations=10000, **extra).sample(case) for _ in range(3)]
        torch.cuda.synchronize()
        for (a, b), (c, d) in zip(got, want):
            assert torch.equal(a, c) and torch.equal(b, d)


def test_arguments_the_rule_does_not_cover_are_refused():
    with pytest.raises(ValueError):
        augment.DeviceAugment(oversample_foreground=0.5, enforce_label_indices=[1])
    with pytest.raises(ValueError):
        augment.DeviceAugment(oversample_foreground=0.5, crop_mode="center")
    for bad in (dict(oversample_foreground=0), dict(oversample_foreground=1.5),
                dict(oversample_foreground=0.5, foreground_classes=[0]),
                dict(oversample_foreground=0.5, foreground_classes=[32]),
                dict(oversample_foreground=0.5, max_locations=0)):
        with pytest.raises(ValueError):
            augment.DeviceAugment(**bad)


def test_batch_with_elastic_equals_the_per_patch_route(volume):
    img, lab, case = volume
    img2, lab2 = _four_classes((80, 72, 70), seed=1)
    cases = [case, augment.DeviceCase(img2, lab2, DEV)]
    aug = augment.DeviceAugment(scale=0.1, crop_size=48, crop_mode="random", oversample_foreground=0.6, **SPATIAL)
    np.random.seed(12)
    b = aug.batch(cases, 4)
    np.random.seed(12)
    for i in range(4):
        picked = cases[int(np.random.randint(0, len(cases)))]
        image, label = aug.sample(picked)
        assert torch.equal(b["image"][i], image) and torch.equal(b["label"][i], label)


# ------------------------------------------------------------------------------------------------ resident cases
def test_device_case_dataset_keeps_its_cases(tmp_path):
    for i, shape in enumerate([(40, 36, 34), (38, 40, 36)]):
        img, lab = _four_classes(shape, seed=i)
        data.save_case({"case_id": "case_%02d" % i, "affine": np.eye(4), "image": img[..., 0], "label": lab}, tmp_path)
    ds = data.DeviceCaseDataset(tmp_path, DEV, max_locations=100)
    assert len(ds) == 2
    item = ds[1]
    assert set(item) == {"image", "label", "case_id"} and item["case_id"] == "case_01"
    resident = item["image"]
    assert isinstance(resident, augment.DeviceCase) and resident.shape == (38, 40, 36, 1)
    assert item["label"] is resident.label and resident.label.is_cuda
    assert ds[1]["image"] is resident                              # loaded, uploaded and indexed once
    assert resident._index is not None and resident.class_index(100) is resident._index
    assert np.array_equal(resident.label.cpu().numpy(), _four_classes((38, 40, 36), seed=1)[1])
    assert data.DeviceCaseDataset(tmp_path, DEV)[0]["image"]._index is None

    aug = augment.DeviceAugment(scale=0.1, crop_size=24, crop_mode="random", oversample_foreground=0.5, max_locations=100)
    np.random.seed(6)
    loader = torch.utils.data.DataLoader(data.DeviceCaseDataset(tmp_path, DEV, max_locations=100, transform=aug),
                                         num_workers=0, batch_size=2)
    batches = list(loader)
    assert len(batches) == 1
    assert tuple(batches[0]["image"].shape) == (2, 1, 24, 24, 24) and batches[0]["image"].is_cuda
    assert tuple(batches[0]["label"].shape) == (2, 24, 24, 24) and batches[0]["label"].dtype == torch.int64
    assert batches[0]["label"].is_cuda and list(batches[0]["case_id"]) == ["case_00", "case_01"]
