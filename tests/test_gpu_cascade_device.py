"""The cascade with every intermediate in HBM (`cascade_predict_case(..., on_device=True)`) against the host route
(`on_device=False`: scipy labelling, numpy float64 merge) on the same models and case, voxel for voxel, and the two merge
kernels against the numpy arithmetic of trainer.cascade_predict_case.  `-m gpu` only."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no HIP device", allow_module_level=True)

import components  # noqa: E402
import data  # noqa: E402
import network  # noqa: E402
import trainer as T  # noqa: E402

DEV = torch.device("cuda:0")


def _g9(golden_dir, detail_classes=3):
    z = np.load(os.path.join(golden_dir, "g9_cascade.npz"))
    torch.manual_seed(3)                                   # the one-class detail model has no fixture weights
    coarse = network.ResUnet3D(num_pool=2, num_features=4, in_channels=1, out_channels=1)
    detail = network.ResUnet3D(num_pool=2, num_features=4, in_channels=1, out_channels=detail_classes)
    coarse.load_state_dict({k[len("coarse/w/"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("coarse/w/")})
    if detail_classes == 3:
        detail.load_state_dict({k[len("detail/w/"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("detail/w/")})
    stats = dict(zip(("mean", "std", "pct_00_5", "pct_99_5"), (float(v) for v in z["stats"])))
    args = lambda c, d: (c, tuple(z["params"][0]), stats, tuple(int(v) for v in z["patches"][0]),
                         d, tuple(z["params"][1]), stats, tuple(int(v) for v in z["patches"][1]))
    kw = dict(step_per_patch=int(z["scalars"][0]), region_threshold=int(z["scalars"][1]), crop_padding=int(z["scalars"][2]),
              verbose=False)
    return z, coarse.to(DEV).eval(), detail.to(DEV).eval(), args, kw


def _both_routes(case, args, kw):
    host = T.cascade_predict_case(dict(case), *args, on_device=False, **kw)
    dev = T.cascade_predict_case(dict(case), *args, on_device=True, **kw)
    assert sorted(host) == sorted(dev)
    for k in host:
        assert type(host[k]) is type(dev[k]), k
        if isinstance(host[k], np.ndarray):
            assert host[k].dtype == dev[k].dtype and host[k].shape == dev[k].shape, k
    assert isinstance(dev["image"], np.ndarray) and np.array_equal(dev["image"], case["image"])
    assert np.array_equal(host["affine"], dev["affine"])
    differing = int((host["pred"] != dev["pred"]).sum())
    assert differing == 0, "%d voxels differ between the two routes" % differing
    return host, dev


def test_g9_device_route_equals_host_route(golden_dir, monkeypatch):
    z, coarse, detail, args, kw = _g9(golden_dir)
    case = {"case_id": "g9", "image": z["image"], "affine": z["affine"]}
    host, dev = _both_routes(case, args(coarse, detail), kw)
    assert dev["pred"].max() >= 1
    # on_device=None: HIP models take the device route, RU3D_CASCADE_DEVICE=0 the host route
    taken = []
    real = T._cascade_predict_case_device
    monkeypatch.setattr(T, "_cascade_predict_case_device", lambda *a, **k: (taken.append(1), real(*a, **k))[1])
    auto = T.cascade_predict_case(dict(case), *args(coarse, detail), **kw)
    assert taken == [1] and np.array_equal(auto["pred"], host["pred"])
    monkeypatch.setenv("RU3D_CASCADE_DEVICE", "0")
    off = T.cascade_predict_case(dict(case), *args(coarse, detail), **kw)
    assert taken == [1] and np.array_equal(off["pred"], host["pred"])


def _synthetic_coarse(shape):
    """Coarse mask with three regions above the threshold (two whose padded boxes overlap, one in a corner whose box
    leaves the volume on two sides) and one component below it."""
    m = np.zeros(shape, np.uint8)
    m[30:50, 20:40, 20:40] = 1
    m[56:72, 30:52, 24:44] = 1
    m[0:10, 0:12, 30:44] = 1
    m[80:83, 70:73, 5:8] = 1
    return m


def test_synthetic_case_overlap_clipping_and_small_component(golden_dir, monkeypatch):
    z, coarse, detail, args, kw = _g9(golden_dir)
    shape = (96, 80, 64)
    rng = np.random.RandomState(4)
    image = (rng.rand(*shape, 1) * 200 - 100).astype(np.float32)
    case = {"case_id": "syn", "image": image, "affine": np.diag([1.6, 1.6, 3.0, 1.0])}
    coarse_mask = _synthetic_coarse(shape)
    real = T.predict_case

    def predict_case(c, model, *a, **k):                 # the coarse stage returns the constructed mask on either route
        if model is coarse:
            c["pred"] = torch.from_numpy(coarse_mask).to(DEV) if k.get("return_device") else coarse_mask.copy()
            c["affine"] = np.asarray(c["affine"], dtype=np.float64)
            return c
        return real(c, model, *a, **k)

    monkeypatch.setattr(T, "predict_case", predict_case)
    kw = dict(kw, region_threshold=1000, crop_padding=10)
    regions = data.regions_crop_case(dict(case, pred=coarse_mask), 1000, 10, "pred")
    boxes = [r["bbox"] for r in regions]
    assert len(boxes) == 3
    assert (boxes[0][:, 0] < 0).sum() == 2                                             # leaves the volume on two sides
    assert all(boxes[1][d][1] > boxes[2][d][0] and boxes[2][d][1] > boxes[1][d][0] for d in range(3))     # overlap
    host, dev = _both_routes(case, args(coarse, detail), kw)
    assert dev["pred"].shape == shape


def test_single_class_detail_model_rounds(golden_dir):
    z, coarse, detail, args, kw = _g9(golden_dir, detail_classes=1)
    case = {"case_id": "g9", "image": z["image"], "affine": z["affine"]}
    host, dev = _both_routes(case, args(coarse, detail), kw)
    assert set(np.unique(dev["pred"]).tolist()) <= {0, 1}


def test_no_region_gives_an_empty_mask(golden_dir):
    z, coarse, detail, args, kw = _g9(golden_dir)
    case = {"case_id": "g9", "image": z["image"], "affine": z["affine"]}
    kw = dict(kw, region_threshold=10 ** 9)                # every component is too small: no region at all
    host, dev = _both_routes(case, args(coarse, detail), kw)
    assert dev["pred"].shape == z["image"].shape[:-1] and dev["pred"].dtype == np.uint8 and not dev["pred"].any()


@pytest.mark.parametrize("classes", [1, 3, 4])
def test_accumulate_and_merge_against_numpy(classes):
    rng = np.random.RandomState(classes)
    shape = (33, 29, 70)
    total = np.zeros(shape + (classes,))
    hits = np.zeros_like(total)
    acc = components.CascadeAccumulator(shape, classes, DEV)
    boxes = [((-4, 20), (-3, 18), (5, 60)), ((10, 40), (8, 33), (-2, 72)), ((12, 30), (0, 29), (30, 64))]
    for bbox in boxes:
        size = tuple(b[1] - b[0] for b in bbox)
        prob = rng.rand(*size, classes).astype(np.float32)
        prob[rng.rand(*size) < 0.05] = np.nan              # rows no window reached
        if classes > 1:
            prob[::3, ::2, ::5, 1] = prob[::3, ::2, ::5, 0]        # exact ties: the first maximum must win
        inside = tuple(slice(max(-bbox[d][0], 0), size[d] - max(bbox[d][1] - shape[d], 0)) for d in range(3))
        target = tuple(slice(max(bbox[d][0], 0), min(bbox[d][1], shape[d])) for d in range(3))
        total[target] += prob[inside]
        hits[target] += 1
        acc.add(torch.from_numpy(prob).to(DEV), [b[0] for b in bbox])
    acc.add(torch.ones((10, 5, 5, classes), dtype=torch.float32, device=DEV), (40, 0, 0))     # misses the volume: no-op
    assert np.array_equal(acc.hits.cpu().numpy(), hits[..., 0].astype(np.int32))
    assert np.array_equal(acc.total.cpu().numpy(), total, equal_nan=True)
    seen = hits > 0
    total[seen] = total[seen] / hits[seen]
    with np.errstate(invalid="ignore"):
        if classes == 1:
            merged = np.nan_to_num(np.around(np.squeeze(total, axis=-1)), nan=0.0)
        else:
            e = np.exp(total - total.max(axis=-1, keepdims=True))
            merged = np.argmax(e / e.sum(axis=-1, keepdims=True), axis=-1)
    got = acc.merge().cpu().numpy()
    assert got.dtype == np.uint8 and np.array_equal(got, merged.astype(np.uint8))
