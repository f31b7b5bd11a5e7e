"""Connected-component labelling, statistics and filtering on the HIP path (csrc/components.hip) against scipy on the
same mask.  Every comparison is exact: the device labels must be `scipy.ndimage.label`'s labels element for element
(same numbering, not a permutation), the sizes `np.bincount`'s, the boxes `ndi.find_objects`'.  `-m gpu` only."""
import ctypes
import os

import numpy as np
import pytest
import scipy.ndimage as ndi
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no HIP device", allow_module_level=True)

import _native as N  # noqa: E402
import components  # noqa: E402
import data  # noqa: E402
import transform  # noqa: E402

DEV = torch.device("cuda:0")


def _check(mask):
    """labels, K, sizes and boxes of `mask` (numpy) from the device against scipy."""
    want, k = ndi.label(mask)
    labels, count = transform.label_components(torch.from_numpy(np.ascontiguousarray(mask)).to(DEV))
    assert labels.dtype == torch.int32 and labels.is_cuda and tuple(labels.shape) == mask.shape
    got = labels.cpu().numpy()
    assert count == k
    assert np.array_equal(got, want)
    sizes, boxes = components.stats(labels, count)
    assert np.array_equal(sizes.cpu().numpy(), np.bincount(want.ravel(), minlength=k + 1)[1:])
    want_boxes = np.array([[v for s in sl for v in (s.start, s.stop)] for sl in ndi.find_objects(want)],
                          dtype=np.int32).reshape(k, 6)
    assert np.array_equal(boxes.cpu().numpy(), want_boxes)
    return labels, count


@pytest.mark.parametrize("density", [0.05, 0.3, 0.6, 0.9])
def test_speckle_densities(density):
    rng = np.random.RandomState(int(density * 100))
    _check((rng.rand(40, 72, 130) < density).astype(np.uint8))


@pytest.mark.parametrize("shape", [(37, 50, 91), (1, 1, 300), (130, 67, 300), (5, 1, 1)])
def test_shapes_that_fit_no_tile(shape):
    rng = np.random.RandomState(sum(shape))
    _check((rng.rand(*shape) < 0.45).astype(np.uint8))


def test_all_zeros_all_ones_checkerboard_and_other_bytes():
    labels, count = _check(np.zeros((20, 17, 70), np.uint8))
    assert count == 0 and not labels.any()
    _check(np.ones((20, 17, 70), np.uint8))
    x, y, z = np.indices((18, 20, 66))
    board = ((x + y + z) % 2 == 0).astype(np.uint8)
    _, count = _check(board)
    assert count == board.size // 2
    rng = np.random.RandomState(5)
    vol = (rng.rand(24, 24, 80) < 0.5) * rng.randint(1, 256, (24, 24, 80))       # foreground bytes 1..255
    _check(vol.astype(np.uint8))
    _check(rng.rand(24, 24, 80) < 0.5)                                          # bool
    _check(((rng.rand(24, 24, 80) < 0.5) * 7).astype(np.int64))                 # any dtype: non-zero is foreground


def test_comb_and_u_shapes_merge_late():
    comb = np.array([[1, 0, 0, 1, 0, 0, 1], [1, 0, 0, 0, 0, 0, 1], [1, 0, 1, 1, 1, 0, 1], [1, 0, 0, 0, 0, 0, 1],
                     [1, 1, 1, 1, 1, 1, 1]], dtype=np.uint8)
    labels, count = transform.label_components(torch.from_numpy(comb).to(DEV))      # two axes: a [1, 5, 7] volume
    assert count == 3 and np.array_equal(labels.cpu().numpy(), ndi.label(comb)[0])
    big = np.kron(comb, np.ones((20, 30), np.uint8))[None].repeat(9, axis=0)         # the comb across many tiles
    big = np.ascontiguousarray(big.transpose(1, 0, 2))
    _check(big)


def _serpentine(shape):
    """A one-voxel-wide path that runs the whole of z, steps two voxels in y, runs back, and at the end of a slab
    moves two voxels in x: one component that crosses every tile many times."""
    X, Y, Z = shape
    vol = np.zeros(shape, np.uint8)
    ys = list(range(0, Y, 2))
    z_at = 0                                            # where the walker stands along z
    for x in range(0, X, 2):
        for n, y in enumerate(ys):
            vol[x, y, :] = 1
            z_at = Z - 1 - z_at
            if n + 1 < len(ys):
                vol[x, min(y, ys[n + 1]):max(y, ys[n + 1]) + 1, z_at] = 1
        if x + 2 < X:
            vol[x:x + 3, ys[-1], z_at] = 1
        ys.reverse()
    return vol


def test_serpentine_through_every_tile():
    vol = _serpentine((64, 64, 256))
    assert ndi.label(vol)[1] == 1
    _check(vol)


def test_two_runs_give_identical_bytes():
    rng = np.random.RandomState(11)
    mask = torch.from_numpy((rng.rand(70, 90, 200) < 0.55).astype(np.uint8)).to(DEV)
    a, ka = transform.label_components(mask)
    b, kb = transform.label_components(mask)
    assert ka == kb and torch.equal(a, b)


def test_large_volume_blobs_plus_speckle():
    rng = np.random.RandomState(2)
    shape = (512, 512, 256)
    vol = rng.rand(*shape) < 0.001
    x, y, z = np.ogrid[:shape[0], :shape[1], :shape[2]]
    vol |= ((x - 150) / 90.0) ** 2 + ((y - 260) / 120.0) ** 2 + ((z - 120) / 70.0) ** 2 < 1
    vol |= ((x - 380) / 80.0) ** 2 + ((y - 250) / 110.0) ** 2 + ((z - 130) / 75.0) ** 2 < 1
    vol = vol.astype(np.uint8)
    want, k = ndi.label(vol)
    labels, count = transform.label_components(torch.from_numpy(vol).to(DEV))
    assert count == k and torch.equal(labels.cpu(), torch.from_numpy(want))
    sizes, boxes = components.stats(labels, count)
    assert np.array_equal(sizes.cpu().numpy(), np.bincount(want.ravel())[1:])
    want_boxes = np.array([[v for s in sl for v in (s.start, s.stop)] for sl in ndi.find_objects(want)], dtype=np.int32)
    assert np.array_equal(boxes.cpu().numpy(), want_boxes)


@pytest.mark.parametrize("threshold", [0, 1, 50, 10000])
def test_remove_small_region_in_place(threshold):
    rng = np.random.RandomState(7)
    vol = rng.rand(48, 60, 100) < 0.3
    vol[5:40, 8:50, 10:90] |= rng.rand(35, 42, 80) < 0.8         # one component far above 10000 voxels
    for dtype in (np.uint8, np.int64, np.bool_):
        host = vol.astype(dtype) * (3 if dtype != np.bool_ else 1)
        host = host.astype(dtype)
        dev = torch.from_numpy(host.copy()).to(DEV)
        want = transform.remove_small_region(host.copy(), threshold)
        out = transform.remove_small_region(dev, threshold)
        assert out is dev and np.array_equal(dev.cpu().numpy(), want)
    case = transform.RemoveSmallRegion(threshold)({"label": torch.from_numpy(vol.astype(np.uint8)).to(DEV)})
    assert np.array_equal(case["label"].cpu().numpy(), transform.remove_small_region(vol.astype(np.uint8), threshold))


def test_filter_renumbers_survivors_like_a_second_labelling():
    rng = np.random.RandomState(9)
    vol = (rng.rand(30, 40, 70) < 0.35).astype(np.uint8)
    mask = torch.from_numpy(vol).to(DEV)
    labels, count = components.label(mask)
    sizes, _ = components.stats(labels, count)
    relabelled, kept = components.filter_small(labels, count, sizes, 6, mask=mask, relabel=True)
    want_mask = transform.remove_small_region(vol.copy(), 6)
    want, k = ndi.label(want_mask)
    assert kept == k and np.array_equal(mask.cpu().numpy(), want_mask)
    assert np.array_equal(relabelled.cpu().numpy(), want)


def test_regions_crop_case_on_the_device_matches_g9(golden_dir):
    z = np.load(os.path.join(golden_dir, "g9_cascade.npz"))
    thr, pad = int(z["scalars"][1]), int(z["scalars"][2])
    host_case = {"case_id": "g9", "image": z["image"], "affine": z["affine"], "pred": z["coarse_pred"],
                 "label": z["eval_label"].astype(np.int64)}
    dev_case = dict(host_case, image=torch.from_numpy(z["image"]).to(DEV), pred=torch.from_numpy(z["coarse_pred"]).to(DEV),
                    label=torch.from_numpy(z["eval_label"].astype(np.int64)).to(DEV))
    want = data.regions_crop_case(host_case, thr, pad, "pred")
    got = data.regions_crop_case(dev_case, thr, pad, "pred")
    assert [r["bbox"].tolist() for r in got] == z["regions"].tolist()
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g["case_id"] == w["case_id"] and np.array_equal(g["affine"], w["affine"])
        assert g["bbox"].dtype == w["bbox"].dtype and np.array_equal(g["bbox"], w["bbox"])
        assert g["image"].is_cuda and g["image"].dtype == torch.float32
        assert np.array_equal(g["image"].cpu().numpy(), w["image"])
        assert g["label"].is_cuda and np.array_equal(g["label"].cpu().numpy(), w["label"])
    # a host image beside a device mask is cropped on the host
    mixed = data.regions_crop_case(dict(host_case, pred=dev_case["pred"]), thr, pad, "pred")
    assert all(isinstance(r["image"], np.ndarray) and np.array_equal(r["image"], w["image"]) for r, w in zip(mixed, want))


def test_bad_arguments_are_refused_before_any_launch():
    lib = N.lib
    mask = torch.zeros((8, 8, 8), dtype=torch.uint8, device=DEV)
    labels = torch.full((8, 8, 8), 77, dtype=torch.int32, device=DEV)
    count = torch.full((1,), 77, dtype=torch.int32, device=DEV)
    ws = torch.empty(1 << 16, dtype=torch.uint8, device=DEV).fill_(0xFF)
    st = N.stream(DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    calls = [lib.ru3d_label_components(p(mask), 2048, 1024, 1024, p(labels), p(count), p(ws), ws.numel(), st),
             lib.ru3d_label_components(None, 8, 8, 8, p(labels), p(count), p(ws), ws.numel(), st),
             lib.ru3d_label_components(p(mask), 8, 8, 8, None, p(count), p(ws), ws.numel(), st),
             lib.ru3d_label_components(p(mask), 8, 8, 8, p(labels), p(count), p(ws), 8, st),
             lib.ru3d_component_stats(p(labels), 8, 8, 8, 2, None, None, st),
             lib.ru3d_filter_components(p(labels), 8, 8, 8, 2, None, 1, p(mask), None, p(count), p(ws), ws.numel(), st)]
    for rc in calls:
        assert rc < 0
    assert lib.ru3d_last_error()
    torch.cuda.synchronize()
    assert int(count.item()) == 77 and bool((labels == 77).all())            # nothing ran
    with pytest.raises(N.Ru3dError):
        components.label(torch.zeros((4, 4, 4), dtype=torch.uint8))            # a CPU tensor has no device route
