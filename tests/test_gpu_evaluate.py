"""The confusion table on the HIP path (csrc/morphology.hip) against np.bincount, trainer.evaluate_case /
evaluate_metrics with HIP operands against the same formulas on those counts and against the reference's numbers
(G9, G10), and the cascade that cleans its mask up while it is still in HBM.  Counts and masks are compared exactly.
`-m gpu` only."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no HIP device", allow_module_level=True)

import morphology  # noqa: E402
import network  # noqa: E402
import trainer as T  # noqa: E402
import transform  # noqa: E402

DEV = torch.device("cuda:0")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _want(pred, label, C):
    p = np.minimum(pred.astype(np.int64), C).ravel()
    g = np.minimum(label.astype(np.int64), C).ravel()
    return np.bincount(g * (C + 1) + p, minlength=(C + 1) ** 2).reshape(C + 1, C + 1)


def _check(pred, label, C):
    got = morphology.confusion(pred, label, C)
    assert got.dtype == torch.int64 and got.is_cuda and tuple(got.shape) == (C + 1, C + 1)
    want = _want(pred.cpu().numpy(), label.cpu().numpy(), C)
    assert np.array_equal(got.cpu().numpy(), want)
    assert torch.equal(morphology.confusion(pred, label, C), got)             # twice the same table
    return want


# ------------------------------------------------------------------------------------------------ confusion counts
@pytest.mark.parametrize("C", [1, 3, 32])
@pytest.mark.parametrize("n", [1, 15, 16, 17, 255, 4099, 1000003])
def test_confusion_equals_bincount(n, C):
    rng = np.random.RandomState(n % 1000 + C)
    pred = _dev(rng.randint(0, C + 3, size=n).astype(np.uint8))               # values above C in either operand
    label = _dev(rng.randint(0, C + 2, size=n).astype(np.uint8))
    want = _check(pred, label, C)
    assert want.sum() == n
    if n > 1000:
        assert want[C].sum() > 0 and want[:, C].sum() > 0


def test_confusion_of_smooth_volumes_and_high_bytes():
    """Long runs of equal pairs (what a segmentation looks like) and bytes up to 255."""
    x, y, z = np.ogrid[:64, :80, :96]
    label = ((x > 20).astype(np.uint8) + (y > 30) + (z > 50)).astype(np.uint8)
    pred = np.roll(label, 3, axis=1)
    pred[:4] = 255
    label[60:] = 200
    _check(_dev(pred), _dev(label), 3)
    _check(_dev(pred), _dev(label), 32)
    zeros = torch.zeros(100000, dtype=torch.uint8, device=DEV)
    assert int(morphology.confusion(zeros, zeros, 2)[0, 0]) == 100000


@pytest.mark.parametrize("offsets", [(1, 1), (3, 3), (0, 5), (7, 2), (16, 0)])
def test_confusion_of_unaligned_views(offsets):
    rng = np.random.RandomState(sum(offsets))
    n = 70001
    a = _dev(rng.randint(0, 5, size=n + 32).astype(np.uint8))
    b = _dev(rng.randint(0, 5, size=n + 32).astype(np.uint8))
    pred, label = a[offsets[0]:offsets[0] + n], b[offsets[1]:offsets[1] + n]
    assert (pred.data_ptr() - label.data_ptr()) % 16 == (offsets[0] - offsets[1]) % 16
    _check(pred, label, 4)
    _check(pred[:9], label[:9], 4)                                            # shorter than the way to a 16-byte boundary


def test_confusion_of_one_large_case():
    n = 67108864 + 7                                                          # 512 x 512 x 256 and a tail
    g = torch.Generator(device=DEV)
    g.manual_seed(5)
    label = torch.randint(0, 4, (n,), generator=g, device=DEV, dtype=torch.uint8)
    pred = torch.where(torch.rand(n, generator=g, device=DEV) < 0.9, label, torch.randint(0, 5, (n,), generator=g, device=DEV,
                                                                                         dtype=torch.uint8))
    want = _check(pred, label, 3)
    assert want.sum() == n


# ------------------------------------------------------------------------------------------------ evaluate_case / metrics
def _dice_from_counts(table, c):
    tp = int(table[c, c])
    fn, fp = int(table[c].sum()) - tp, int(table[:, c].sum()) - tp
    return (tp + 1e-7) / (tp + 0.5 * fn + 0.5 * fp + 1e-7)


def test_evaluate_case_with_hip_operands(golden_dir):
    z = np.load(os.path.join(golden_dir, "g9_cascade.npz"))
    pred, label = z["pred"], z["eval_label"]
    host = T.evaluate_case({"pred": pred, "label": label})
    table = _want(pred, label, 32)
    exact = [_dice_from_counts(table, c) for c in range(1, int(label.max()) + 1)]
    for case in ({"pred": _dev(pred), "label": _dev(label)}, {"pred": _dev(pred), "label": label},
                 {"pred": pred, "label": _dev(label)}, {"pred": _dev(pred), "label": label.astype(np.int64)},
                 {"pred": _dev(pred).to(torch.int32), "label": _dev(label)}):
        got = T.evaluate_case(case)
        assert all(isinstance(v, float) for v in got)
        assert got == exact                                                   # the float64 formula on the integer counts
        assert np.allclose(got, host, rtol=0, atol=1e-6)                      # the numpy route sums in float32
        assert np.allclose(got, z["eval_dice"], rtol=0, atol=1e-6)
    assert torch.is_tensor(case["pred"]) and case["pred"].is_cuda             # the case is left as it was


def test_evaluate_case_rules_on_the_device():
    label = np.zeros((4, 5, 6), np.uint8)
    label[0] = 3                                                              # classes 1 and 2 are absent: Dice of empty vs pred
    pred = np.zeros_like(label)
    pred[0, :2] = 3
    pred[1] = 40                                                              # a prediction class the label lacks is no error
    got = T.evaluate_case({"pred": _dev(pred), "label": _dev(label)})
    assert len(got) == 3 and got[0] == 1.0 and got[1] == 1.0 and got[2] == (12 + 1e-7) / (12 + 0.5 * 18 + 1e-7)
    assert np.allclose(got, T.evaluate_case({"pred": pred, "label": label}), rtol=0, atol=1e-6)
    assert T.evaluate_case({"pred": _dev(pred), "label": _dev(np.zeros_like(label))}) == []
    label[3] = 32
    with pytest.raises(ValueError, match="above 31"):
        T.evaluate_case({"pred": _dev(pred), "label": _dev(label)})
    label[3] = 31
    assert len(T.evaluate_case({"pred": _dev(pred), "label": _dev(label)})) == 31


def test_evaluate_metrics_with_hip_operands(golden_dir):
    z = np.load(os.path.join(golden_dir, "g10_post.npz"))
    host = T.evaluate_metrics({"pred": z["pred"], "label": z["label"]})
    for case in ({"pred": _dev(z["pred"]), "label": _dev(z["label"])}, {"pred": z["pred"], "label": _dev(z["label"])}):
        got = T.evaluate_metrics(case)
        assert got == host                                                    # both routes: Python floats on integer counts
        table = np.array([[m["dsc"], m["sen"], m["spe"], m["acc"]] for m in got])
        assert np.allclose(table, z["metrics"], rtol=0, atol=1e-6)


# ------------------------------------------------------------------------------------------------ cascade + clean-up in HBM
def _g9(golden_dir):
    z = np.load(os.path.join(golden_dir, "g9_cascade.npz"))
    coarse = network.ResUnet3D(num_pool=2, num_features=4, in_channels=1, out_channels=1)
    detail = network.ResUnet3D(num_pool=2, num_features=4, in_channels=1, out_channels=3)
    coarse.load_state_dict({k[len("coarse/w/"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("coarse/w/")})
    detail.load_state_dict({k[len("detail/w/"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("detail/w/")})
    stats = dict(zip(("mean", "std", "pct_00_5", "pct_99_5"), (float(v) for v in z["stats"])))
    args = (coarse.to(DEV).eval(), tuple(z["params"][0]), stats, tuple(int(v) for v in z["patches"][0]),
            detail.to(DEV).eval(), tuple(z["params"][1]), stats, tuple(int(v) for v in z["patches"][1]))
    kw = dict(step_per_patch=int(z["scalars"][0]), region_threshold=int(z["scalars"][1]), crop_padding=int(z["scalars"][2]),
              verbose=False)
    return z, args, kw


def test_cascade_cleans_its_mask_up_in_hbm(golden_dir):
    z, args, kw = _g9(golden_dir)
    case = {"case_id": "g9", "image": z["image"], "affine": z["affine"]}
    plain = T.cascade_predict_case(dict(case), *args, on_device=False, **kw)["pred"]
    label = int(np.bincount(plain.ravel(), minlength=4)[1:].argmax()) + 1     # the class the fixture's models predict most
    sizes = np.bincount(transform.label_components(plain > 0)[0].ravel())[1:]
    threshold = int(sizes.max())                                              # keeps the largest component only
    post = functools.partial(transform.post_transform, threshold=threshold, label=label, structure=np.ones((3, 3, 3)))
    want = post(plain.copy())
    assert (want != plain).any() and want.any(), "the clean-up must change some voxels and keep some"

    dev = T.cascade_predict_case(dict(case), *args, on_device=True, post_transform=post, return_device=True, **kw)
    assert torch.is_tensor(dev["pred"]) and dev["pred"].is_cuda and dev["pred"].dtype == torch.uint8
    assert np.array_equal(dev["pred"].cpu().numpy(), want)
    down = T.cascade_predict_case(dict(case), *args, on_device=True, post_transform=post, **kw)
    assert isinstance(down["pred"], np.ndarray) and np.array_equal(down["pred"], want)
    host = T.cascade_predict_case(dict(case), *args, on_device=False, post_transform=post, **kw)
    assert isinstance(host["pred"], np.ndarray) and np.array_equal(host["pred"], want)
    kept = T.cascade_predict_case(dict(case), *args, on_device=True, return_device=True, **kw)
    assert kept["pred"].is_cuda and np.array_equal(kept["pred"].cpu().numpy(), plain)
    with pytest.raises(ValueError, match="return_device"):
        T.cascade_predict_case(dict(case), *args, on_device=False, return_device=True, **kw)
    # evaluation of the device-resident result against the fixture's label: one table, same numbers as the host route
    got = T.evaluate_case({"pred": dev["pred"], "label": z["eval_label"]})
    assert np.allclose(got, T.evaluate_case({"pred": want, "label": z["eval_label"]}), rtol=0, atol=1e-6)
