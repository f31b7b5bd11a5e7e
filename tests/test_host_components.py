"""CPU-only checks of the connected-component / cascade-merge surface: the numpy route of `transform.label_components`
is scipy's labelling with first-voxel numbering, the C ABI declares, exports and binds the new entry points, their
argument checks answer before anything is launched, and the new keywords of the inference drivers exist and resolve to
the host route for CPU models."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import scipy.ndimage as ndi
import torch

import _native as N
import inference as I
import network
import trainer as T
import transform

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("ru3d_components_workspace_bytes", "ru3d_label_components", "ru3d_component_stats",
                "ru3d_filter_components", "ru3d_region_accumulate", "ru3d_cascade_merge")

COMB = np.array([[1, 0, 0, 1, 0, 0, 1],
                 [1, 0, 0, 0, 0, 0, 1],
                 [1, 0, 1, 1, 1, 0, 1],
                 [1, 0, 0, 0, 0, 0, 1],
                 [1, 1, 1, 1, 1, 1, 1]], dtype=np.uint8)
COMB_LABELS = np.array([[1, 0, 0, 2, 0, 0, 1],
                        [1, 0, 0, 0, 0, 0, 1],
                        [1, 0, 3, 3, 3, 0, 1],
                        [1, 0, 0, 0, 0, 0, 1],
                        [1, 1, 1, 1, 1, 1, 1]], dtype=np.int32)


def test_label_components_numpy_route_is_scipy_with_first_voxel_numbering():
    labels, count = transform.label_components(COMB)
    assert count == 3 and isinstance(count, int)
    assert np.array_equal(labels, COMB_LABELS)          # the two arms of the comb merge late and still carry label 1
    rng = np.random.RandomState(3)
    vol = rng.rand(9, 11, 13) < 0.4
    labels, count = transform.label_components(vol)
    want, k = ndi.label(vol)
    assert count == k and np.array_equal(labels, want)
    firsts = [np.flatnonzero(labels.ravel() == i + 1)[0] for i in range(count)]
    assert firsts == sorted(firsts)
    # a volume with the comb as one slice: same numbering in 3D
    labels, count = transform.label_components(COMB[None])
    assert count == 3 and np.array_equal(labels[0], COMB_LABELS)


def test_remove_small_region_numpy_route_unchanged():
    vol = np.zeros((6, 6, 6), dtype=np.uint8)
    vol[0, 0, :3] = 1
    vol[3:, 3:, 3:] = 1
    out = transform.remove_small_region(vol, 4)
    assert out is vol and vol[0, 0].sum() == 0 and vol.sum() == 27
    case = transform.RemoveSmallRegion(28)({"label": vol})
    assert case["label"].sum() == 0


def test_header_library_and_bindings_name_the_component_entry_points():
    text = open(os.path.join(ROOT, "include", "ru3d.h")).read()
    raw = ctypes.CDLL(N.LIB_PATH)
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert hasattr(raw, name), name
        assert name in N.SIGNATURES, name
    assert "components.hip" in open(os.path.join(ROOT, "3d-unet-renal-anatomy-extraction_amd", "csrc", "Makefile")).read()


def test_component_argument_checks_answer_before_any_launch():
    lib = N.lib
    assert lib.ru3d_components_workspace_bytes(64, 64, 64) >= 64 * 64 * 8 + 128 * 4
    assert lib.ru3d_components_workspace_bytes(2048, 1024, 1024) == 0          # 2^31 voxels
    assert lib.ru3d_components_workspace_bytes(0, 4, 4) == 0
    fake = ctypes.c_void_p(4096)                                                # never dereferenced on these paths
    rc = lib.ru3d_label_components(fake, 2048, 1024, 1024, fake, fake, fake, 1 << 40, None)
    assert rc < 0 and b"2^31" in lib.ru3d_last_error()
    rc = lib.ru3d_label_components(None, 8, 8, 8, fake, fake, fake, 1 << 20, None)
    assert rc < 0 and b"label_components" in lib.ru3d_last_error()
    rc = lib.ru3d_label_components(fake, 8, 8, 8, fake, fake, fake, 16, None)
    assert rc < 0 and b"workspace" in lib.ru3d_last_error()
    rc = lib.ru3d_component_stats(None, 8, 8, 8, 3, fake, fake, None)
    assert rc < 0 and b"component_stats" in lib.ru3d_last_error()
    rc = lib.ru3d_filter_components(fake, 8, 8, 8, 3, fake, 1, None, None, fake, fake, 1 << 20, None)
    assert rc < 0 and b"filter_components" in lib.ru3d_last_error()
    rc = lib.ru3d_region_accumulate(fake, 4, 4, 4, 9, 0, 0, 0, fake, fake, 8, 8, 8, None)
    assert rc < 0 and b"classes" in lib.ru3d_last_error()
    rc = lib.ru3d_cascade_merge(fake, None, 8, 8, 8, 3, fake, None)
    assert rc < 0 and b"cascade_merge" in lib.ru3d_last_error()


def test_new_keywords_exist_and_default_to_todays_behaviour():
    sig = inspect.signature(T.cascade_predict_case)
    assert list(sig.parameters)[-1] == "on_device" and sig.parameters["on_device"].default is None
    assert inspect.signature(T.cascade_predict).parameters["on_device"].default is None
    assert inspect.signature(T.batch_cascade_predict).parameters["on_device"].default is None
    assert inspect.signature(I.predict_case).parameters["return_device"].default is False
    assert T.predict_case is I.predict_case


def test_cpu_models_resolve_to_the_host_route(monkeypatch):
    coarse = network.ResUnet3D(num_pool=1, num_features=2, in_channels=1, out_channels=1)
    detail = network.ResUnet3D(num_pool=1, num_features=2, in_channels=1, out_channels=3)
    assert not T._models_on_hip(coarse, detail)
    calls = []

    def host_predict_case(case, model, *a, **kw):
        calls.append(kw)
        case["pred"] = np.zeros(case["image"].shape[:-1], dtype=np.uint8)      # empty coarse mask: no region
        return case

    monkeypatch.setattr(T, "predict_case", host_predict_case)
    monkeypatch.setattr(T, "_cascade_predict_case_device",
                        lambda *a, **k: pytest.fail("CPU models must not take the device route"))
    case = {"case_id": "c", "image": np.zeros((6, 5, 4, 1), np.float32), "affine": np.eye(4)}
    out = T.cascade_predict_case(case, coarse, (1, 1, 1), {}, (4, 4, 4), detail, (1, 1, 1), {}, (4, 4, 4), verbose=False)
    assert out["pred"].shape == (6, 5, 4) and out["pred"].dtype == np.uint8 and not out["pred"].any()
    assert len(calls) == 1 and "return_device" not in calls[0]
