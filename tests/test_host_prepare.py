"""CPU-only checks of the dataset-preparation feature: the five batch drivers of data.py on a temporary folder of small
synthetic NIfTI cases (host route), the declarations of the new entry points and their argument checks.

The reference's data.py cannot be imported where this suite is built (nibabel and transforms3d are absent), so there is
no golden fixture from it for these functions: the yardstick for `analyze_cases` / `analyze_raw_cases` is the numpy
restatement written out in this file (`np.concatenate([img[lab > 0][::10] ...])`, `np.median`, `np.percentile`, ...),
and for the other drivers the per-case functions test_host_data.py already pins."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import _native as N
import data
import nifti
from utils import json_load, json_save

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["ru3d_threshold_bbox", "ru3d_masked_sample_workspace_bytes", "ru3d_masked_sample",
                "ru3d_order_stats_workspace_bytes", "ru3d_order_stats", "ru3d_moments_workspace_bytes", "ru3d_moments"]
REFERENCE_SIGNATURES = {
    "batch_load_crop_case": ["image_dir", "label_dir", "save_dir", "air", "data_range"],
    "analyze_cases": ["load_dir", "props_file", "data_range"],
    "analyze_raw_cases": ["image_dir", "label_dir", "props_file", "data_range"],
    "batch_resample_normalize_case": ["load_dir", "save_dir", "target_spacing", "normalize_stats", "data_range"],
    "batch_regions_crop_case": ["load_dir", "save_dir", "threshold", "padding", "pred_dir", "data_range"],
}


def test_the_five_drivers_keep_the_reference_signatures():
    for name, params in REFERENCE_SIGNATURES.items():
        sig = inspect.signature(getattr(data, name))
        names = list(sig.parameters)
        assert names[:len(params)] == params, name
        assert names[-1] == "device" and sig.parameters["device"].default is None, name
        extra = names[len(params):-1]
        assert extra == (["sample_stride"] if name.startswith("analyze") else []), name
    assert inspect.signature(data.analyze_cases).parameters["sample_stride"].default == 10
    assert inspect.signature(data.batch_load_crop_case).parameters["air"].default == -200
    assert inspect.signature(data.batch_regions_crop_case).parameters["padding"].default == 20
    for name in REFERENCE_SIGNATURES:
        assert name in data.__doc__


# ------------------------------------------------------------------------------------------------ synthetic dataset
def _blob(shape, num_classes, seed, channels=1):
    rng = np.random.RandomState(seed)
    g = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing="ij"), axis=-1).astype(np.float64)
    r = np.sqrt((((g - np.array(shape) / 2.0) / (np.array(shape) / 2.6)) ** 2).sum(axis=-1))
    image = np.where(r < 1, 60 + 200 * (1 - r), -1000)[..., None] + rng.randn(*shape, channels) * 5 + 40 * np.arange(channels)
    image = np.round(image).astype(np.float32)                     # integer-valued like CT
    label = np.zeros(shape, dtype=np.uint8)
    label[r < 0.55] = 1
    if num_classes > 2:
        label[r < 0.3] = 2
    return (image[..., 0] if channels == 1 else image), label


def _write_raw(folder, channels=1):
    images, labels = folder / "imagesTr", folder / "labelsTr"
    images.mkdir(parents=True), labels.mkdir(parents=True)
    plain = np.diag([1.2, 1.5, 2.5, 1.0])
    plain[:3, 3] = [-20.0, 11.0, 5.0]
    for i, (shape, classes) in enumerate([((30, 26, 22), 2), ((24, 28, 20), 2), ((26, 22, 24), 3)]):
        image, label = _blob(shape, classes, 10 + i, channels)
        aff = plain
        if i == 0:                                                 # stored with swapped and flipped axes
            order = (1, 0, 2) + ((3,) if channels > 1 else ())
            image, label = image.transpose(order)[::-1], label.transpose(1, 0, 2)[::-1]
            aff = np.array([[0, 1.2, 0, -20.0], [-1.5, 0, 0, 60.0], [0, 0, 2.5, 5.0], [0, 0, 0, 1.0]])
        nifti.save(np.ascontiguousarray(image), aff, images / ("case_%02d.nii.gz" % i))
        nifti.save(np.ascontiguousarray(label), aff, labels / ("case_%02d.nii.gz" % i))
    return images, labels


def _restated_statistics(samples):
    v = np.concatenate(samples)
    return {"median": np.median(v).item(), "mean": np.mean(v).item(), "std": np.std(v).item(), "min": np.min(v).item(),
            "max": np.max(v).item(), "pct_00_5": np.percentile(v, 0.5).item(), "pct_99_5": np.percentile(v, 99.5).item()}


def _restated_geometry(cases):
    spacings = np.array([data.get_spacing(c["affine"]) for c in cases])
    shapes = np.array([c["image"].shape[:3] for c in cases])
    out = {}
    for name, fn in (("max", np.max), ("min", np.min), ("mean", np.mean), ("median", np.median)):
        out["%s_spacing" % name] = fn(spacings, axis=0).tolist()
        out["%s_shape" % name] = fn(shapes, axis=0).tolist()
    return out


def test_the_preparation_chain_on_a_folder_of_nifti_files(tmp_path):
    images, labels = _write_raw(tmp_path / "raw")
    crop, norm, region, region_p = (tmp_path / n for n in ("crop", "norm", "region", "region_p"))

    # 1. crop
    data.batch_load_crop_case(images, labels, crop, -200)
    names = sorted(p.name for p in crop.iterdir())
    assert names == [n % i for i in range(3) for n in ("case_%02d.image.nii.gz", "case_%02d.label.nii.gz")]
    cases = data.CaseDataset(crop)
    raw0 = data.load_case(images / "case_00.nii.gz", labels / "case_00.nii.gz")
    want0 = data.orient_crop_case(raw0, -200)
    assert np.array_equal(cases[0]["image"], want0["image"]) and np.array_equal(cases[0]["label"], want0["label"])
    assert cases[0]["image"].shape[0] < raw0["image"].shape[1]      # reoriented (axes swapped back) and the air margin cut
    assert np.allclose(data.get_spacing(cases[0]["affine"]), (1.2, 1.5, 2.5), atol=1e-6)
    partial = tmp_path / "crop_partial"
    data.batch_load_crop_case(images, labels, partial, data_range=[2])
    assert sorted(p.name for p in partial.iterdir()) == ["case_02.image.nii.gz", "case_02.label.nii.gz"]

    # 2. analyse: the ten-line numpy restatement
    loaded = [cases[i] for i in range(3)]
    props = data.analyze_cases(crop)
    want = _restated_geometry(loaded)
    want["modality_statstics"] = [_restated_statistics([c["image"][..., 0][c["label"] > 0][::10] for c in loaded])]
    assert props == want
    assert set(props["modality_statstics"][0]) == {"median", "mean", "std", "min", "max", "pct_00_5", "pct_99_5"}
    assert all(type(v) is float for v in props["modality_statstics"][0].values())
    every = data.analyze_cases(crop, sample_stride=1)
    assert every["modality_statstics"] == [_restated_statistics([c["image"][..., 0][c["label"] > 0] for c in loaded])]
    assert every["modality_statstics"] != props["modality_statstics"]
    two = data.analyze_cases(crop, data_range=range(2))
    assert two["modality_statstics"] == [_restated_statistics([c["image"][..., 0][c["label"] > 0][::10] for c in loaded[:2]])]
    assert two["max_shape"] == _restated_geometry(loaded[:2])["max_shape"]
    props_file = tmp_path / "props.json"
    json_save(str(props_file), {"air": -200, "median_shape": "stale"})
    assert data.analyze_cases(crop, props_file) == props
    merged = json_load(str(props_file))
    assert merged["air"] == -200 and merged["median_shape"] == props["median_shape"]
    assert merged["modality_statstics"] == props["modality_statstics"]
    with pytest.raises(ValueError):
        data.analyze_cases(crop, sample_stride=0)

    # 3. region crop, on the label and on a prediction folder
    data.batch_regions_crop_case(crop, region, threshold=50, padding=4)
    want_regions = [r for c in loaded for r in data.regions_crop_case(c, 50, 4)]
    assert len(want_regions) == 3
    assert sorted(p.name for p in region.iterdir()) == sorted(
        "%s.%s.nii.gz" % (r["case_id"], k) for r in want_regions for k in ("image", "label"))
    got_regions = data.CaseDataset(region)
    for i, r in enumerate(want_regions):
        assert got_regions[i]["case_id"] == r["case_id"] and r["case_id"].endswith("_000")
        assert np.array_equal(got_regions[i]["image"], r["image"]) and np.array_equal(got_regions[i]["label"], r["label"])
    pred = tmp_path / "pred"
    for c in loaded[:2]:                                           # a prediction that is half of the label
        half = c["label"].copy()
        half[: half.shape[0] // 2] = 0
        data.save_pred({"case_id": c["case_id"], "affine": c["affine"], "pred": half}, pred)
    data.batch_regions_crop_case(crop, region_p, 50, 4, pred)
    got_p = data.CaseDataset(region_p)
    assert len(got_p) == 2 and not list(region_p.glob("*.pred.nii.gz"))
    for i in range(2):
        assert got_p[i]["image"].shape[0] < got_regions[i]["image"].shape[0]
        with_pred = dict(loaded[i], pred=nifti.load(pred / ("%s.pred.nii.gz" % loaded[i]["case_id"]))[0].astype(np.int64))
        assert np.array_equal(got_p[i]["image"], data.regions_crop_case(with_pred, 50, 4, "pred")[0]["image"])

    # 4. resample and normalise with the statistics just computed
    target = (1.6, 1.6, 2.0)
    data.batch_resample_normalize_case(crop, norm, target, props["modality_statstics"], data_range=range(1, 3))
    got_norm = data.CaseDataset(norm)
    assert len(got_norm) == 2
    for i in range(2):
        want_case = data.resample_normalize_case(loaded[i + 1], target, props["modality_statstics"])
        assert got_norm[i]["case_id"] == loaded[i + 1]["case_id"]
        assert np.array_equal(got_norm[i]["image"], want_case["image"].astype(np.float32))
        assert np.array_equal(got_norm[i]["label"], want_case["label"])
        assert np.allclose(data.get_spacing(got_norm[i]["affine"]), target, atol=1e-5)
        assert abs(float(got_norm[i]["image"][got_norm[i]["label"] > 0].mean())) < 1.0      # normalised foreground


def test_analyze_cases_keeps_one_sample_per_channel(tmp_path):
    """The reference's `[[]*n_modality]` is `[[]]`: two channels raise IndexError there."""
    images, labels = _write_raw(tmp_path / "raw", channels=2)
    data.batch_load_crop_case(images, labels, tmp_path / "crop")
    cases = data.CaseDataset(tmp_path / "crop")
    loaded = [cases[i] for i in range(3)]
    assert loaded[0]["image"].shape[-1] == 2
    props = data.analyze_cases(tmp_path / "crop")
    assert props["modality_statstics"] == [
        _restated_statistics([c["image"][..., ch][c["label"] > 0][::10] for c in loaded]) for ch in range(2)]
    assert props["modality_statstics"][1]["mean"] > props["modality_statstics"][0]["mean"] + 30


def test_analyze_raw_cases(tmp_path):
    images, labels = _write_raw(tmp_path / "raw")
    raw = [data.load_case(images / ("case_%02d.nii.gz" % i), labels / ("case_%02d.nii.gz" % i)) for i in range(3)]
    props_file = tmp_path / "props.json"
    json_save(str(props_file), {"modality": {"0": "CT"}})
    props = data.analyze_raw_cases(images, labels, props_file)
    want = _restated_geometry(raw)
    want["modality_statstics"] = _restated_statistics([c["image"][c["label"] > 0][::10].reshape(-1) for c in raw])
    assert props == want and isinstance(props["modality_statstics"], dict)
    assert json_load(str(props_file)) == {"modality": {"0": "CT"}, **props}
    assert props["max_shape"] == [26, 30, 24]                     # before any crop or reorientation: case 0 is stored transposed
    one = data.analyze_raw_cases(images, labels, data_range=[1], sample_stride=3)
    assert one["modality_statstics"] == _restated_statistics([raw[1]["image"][raw[1]["label"] > 0][::3].reshape(-1)])


# ------------------------------------------------------------------------------------------------ library surface
def test_entry_points_are_declared_built_and_bound():
    header = open(os.path.join(ROOT, "include", "ru3d.h")).read()
    raw = ctypes.CDLL(N.LIB_PATH)
    for name in ENTRY_POINTS:
        assert name + "(" in header, name
        assert hasattr(raw, name), name
        assert name in N.SIGNATURES, name
    csrc = os.path.join(ROOT, "3d-unet-renal-anatomy-extraction_amd", "csrc")
    assert "prepare.hip" in open(os.path.join(csrc, "Makefile")).read()
    assert "prepare.hip" in open(os.path.join(ROOT, "tools", "isa_check.py")).read()
    assert "#define RU3D_ORDER_STATS_MAX_RANKS 8" in header and N.ORDER_STATS_MAX_RANKS == 8
    assert N.lib.ru3d_version() == 201


def test_c_argument_checks_answer_before_any_launch():
    lib = N.lib
    fake = ctypes.c_void_p(4096)                                   # never dereferenced on these paths
    big = 1 << 20

    def failed(rc, word):
        return rc < 0 and word in lib.ru3d_last_error()

    assert failed(lib.ru3d_threshold_bbox(None, 4, 4, 4, 1, -200.0, fake, fake, None), b"null")
    assert failed(lib.ru3d_threshold_bbox(fake, 4, 4, 4, 1, -200.0, None, fake, None), b"null")
    assert failed(lib.ru3d_threshold_bbox(fake, 4, 4, 4, 1, -200.0, fake, None, None), b"null")
    assert failed(lib.ru3d_threshold_bbox(fake, 2048, 1024, 1024, 1, -200.0, fake, fake, None), b"2^31")
    assert failed(lib.ru3d_threshold_bbox(fake, 4, 0, 4, 1, -200.0, fake, fake, None), b"not supported")
    assert failed(lib.ru3d_threshold_bbox(fake, 4, 4, 4, 0, -200.0, fake, fake, None), b"channels")
    assert failed(lib.ru3d_threshold_bbox(fake, 4, 4, 4, 1, float("nan"), fake, fake, None), b"not a number")

    assert lib.ru3d_masked_sample_workspace_bytes(512, 512, 256) >= (512 * 512 * 256 // 2048) * 4
    assert lib.ru3d_masked_sample_workspace_bytes(2048, 1024, 1024) == 0

    def sample(image=fake, shape=(4, 4, 4), C=1, channel=0, label=fake, code=N.LABEL_U8, stride=10, out=fake, capacity=8,
               count=fake, ws=fake, ws_bytes=big):
        return lib.ru3d_masked_sample(image, *shape, C, channel, label, code, stride, out, capacity, count, ws, ws_bytes,
                                      None)

    assert failed(sample(shape=(2048, 1024, 1024)), b"2^31")
    assert failed(sample(image=None), b"null")
    assert failed(sample(label=None), b"null")
    assert failed(sample(count=None), b"null")
    assert failed(sample(ws=None), b"null")
    assert failed(sample(C=2, channel=2), b"channel 2 of 2")
    assert failed(sample(channel=-1), b"channel")
    assert failed(sample(stride=0), b"stride")
    assert failed(sample(code=2), b"label dtype")
    assert failed(sample(capacity=0), b"capacity")
    assert failed(sample(shape=(64, 64, 64), ws_bytes=256), b"workspace")

    ranks = (ctypes.c_int64 * 9)(*range(9))
    assert lib.ru3d_order_stats_workspace_bytes() > 0 and lib.ru3d_moments_workspace_bytes() > 0
    assert failed(lib.ru3d_order_stats(None, 100, ranks, 2, fake, fake, big, None), b"null")
    assert failed(lib.ru3d_order_stats(fake, 100, None, 2, fake, fake, big, None), b"null")
    assert failed(lib.ru3d_order_stats(fake, 100, ranks, 2, None, fake, big, None), b"null")
    assert failed(lib.ru3d_order_stats(fake, 100, ranks, 9, fake, fake, big, None), b"9 ranks")
    assert failed(lib.ru3d_order_stats(fake, 100, ranks, 0, fake, fake, big, None), b"0 ranks")
    assert failed(lib.ru3d_order_stats(fake, 5, ranks, 6, fake, fake, big, None), b"rank 5 of 5")
    assert failed(lib.ru3d_order_stats(fake, 0, ranks, 1, fake, fake, big, None), b"0 values")
    assert failed(lib.ru3d_order_stats(fake, 100, ranks, 2, fake, fake, 64, None), b"workspace")
    assert failed(lib.ru3d_moments(None, 100, fake, fake, big, None), b"null")
    assert failed(lib.ru3d_moments(fake, 100, None, fake, big, None), b"null")
    assert failed(lib.ru3d_moments(fake, 0, fake, fake, big, None), b"0 values")
    assert failed(lib.ru3d_moments(fake, 100, fake, fake, 64, None), b"workspace")
    assert failed(lib.ru3d_moments(ctypes.c_void_p(4098), 100, fake, fake, big, None), b"aligned")
