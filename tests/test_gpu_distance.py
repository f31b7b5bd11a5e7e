"""GPU checks of csrc/distance.hip and what is built on it: the squared distance transform bit for bit against a brute
force of the contract expression and against scipy, the surface of a packed mask, the ordered gather and its
reductions, trainer.evaluate_surface_case on HIP operands against the numpy route, transform.distance_transform_edt on a
HIP tensor, the file round trip, and a prediction the cascade left in HBM."""
import math
import os

import numpy as np
import pytest
import scipy.ndimage as ndi
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no HIP device", allow_module_level=True)

import _native as N  # noqa: E402
import distance  # noqa: E402
import morphology  # noqa: E402
import nifti  # noqa: E402
import trainer  # noqa: E402
import transform  # noqa: E402

DYADIC = [(1.0, 1.0, 1.0), (0.75, 0.75, 3.0)]
ODD = (0.7, 0.83, 3.1)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a HIP device"
    return torch.device("cuda:0")


def contract_brute(features, spacing):
    """out[p] = min over the feature voxels f of fl(A + fl(B + C)), A = fl(fl(sx (px - fx))^2): every pair visited."""
    f = np.argwhere(features)
    if not len(f):
        return np.full(features.shape, np.inf)
    p = np.indices(features.shape).reshape(3, -1).T
    out = np.empty(len(p))
    for i in range(0, len(p), 4096):
        q = p[i:i + 4096]
        a, b, c = ((spacing[k] * (q[:, None, k] - f[None, :, k]).astype(np.float64)) ** 2 for k in range(3))
        out[i:i + 4096] = (a + (b + c)).min(axis=1)
    return out.reshape(features.shape)


def packed(mask, dev):
    return morphology.pack(torch.from_numpy(np.ascontiguousarray(mask)).to(dev))


def edt(mask, spacing, dev):
    return distance.edt_squared(packed(mask, dev), spacing).cpu().numpy()


def ulps(a, b):
    return np.abs(a.view(np.int64) - b.view(np.int64)).max()


# ------------------------------------------------------------------------------------------------ the transform
@pytest.mark.parametrize("spacing", DYADIC + [ODD])
@pytest.mark.parametrize("Z", [1, 63, 64, 65, 130])
def test_edt_squared_is_the_contract_bit_for_bit_across_word_boundaries(dev, spacing, Z):
    rng = np.random.RandomState(Z)
    for density in (0.5, 0.01):
        mask = rng.rand(7, 9, Z) < density
        got = edt(mask, spacing, dev)
        assert got.dtype == np.float64 and np.array_equal(got, contract_brute(mask, spacing)), (Z, density)


@pytest.mark.parametrize("spacing", DYADIC + [ODD])
def test_edt_squared_on_the_special_volumes(dev, spacing):
    assert np.array_equal(edt(np.ones((1, 1, 1), bool), spacing, dev), np.zeros((1, 1, 1)))
    assert np.isinf(edt(np.zeros((1, 1, 1), bool), spacing, dev)).all()
    single = np.zeros((9, 10, 70), bool)
    single[8, 0, 69] = True                                                    # a single feature, in a corner
    assert np.array_equal(edt(single, spacing, dev), contract_brute(single, spacing))
    face = np.zeros((11, 6, 20), bool)
    face[:, 5, :] = np.random.RandomState(2).rand(11, 20) < 0.3                # features on one face only
    assert np.array_equal(edt(face, spacing, dev), contract_brute(face, spacing))
    assert np.isinf(edt(np.zeros((5, 6, 70), bool), spacing, dev)).all()       # no feature at all
    row = np.random.RandomState(3).rand(200) < 0.05                            # a 1-axis volume
    got = distance.edt_squared(packed(row, dev), spacing[2]).cpu().numpy()
    assert got.shape == (200,) and np.array_equal(got, contract_brute(row.reshape(1, 1, -1), spacing).ravel())


@pytest.mark.parametrize("shape", [(160, 160, 80), (300, 40, 70), (40, 600, 33)])
def test_edt_squared_against_scipy_on_larger_volumes(dev, shape):
    # 300 and 600 voxels along x / y: longer than a tile of 16 columns holds (256), so the narrower tilings run too
    rng = np.random.RandomState(shape[0])
    x, y, z = np.ogrid[:shape[0], :shape[1], :shape[2]]
    mask = ((x - shape[0] // 3) ** 2 + (y - shape[1] // 2) ** 2 + (z - shape[2] // 2) ** 2 < (min(shape) // 3) ** 2)
    mask |= rng.rand(*shape) < 0.0005
    for spacing in DYADIC:
        got = np.sqrt(edt(mask, spacing, dev))
        assert np.array_equal(got, ndi.distance_transform_edt(~mask, sampling=spacing)), spacing
    got = np.sqrt(edt(mask, ODD, dev))
    assert ulps(got, ndi.distance_transform_edt(~mask, sampling=ODD)) <= 2
    assert np.isinf(edt(np.zeros(shape, bool), ODD, dev)).all()


def test_far_feature_in_a_corner_of_256x256x128(dev):
    mask = np.zeros((256, 256, 128), bool)
    mask[0, 255, 127] = True
    for spacing in ((1.0, 1.0, 1.0), ODD):
        got = edt(mask, spacing, dev)
        sx, sy, sz = (np.float64(s) for s in spacing)
        assert np.array_equal(got[:, 255, 127], (sx * np.arange(256.0)) ** 2 + (0.0 + 0.0))
        assert np.array_equal(got[0, :, 127], 0.0 + ((sy * (255.0 - np.arange(256.0))) ** 2 + 0.0))
        assert np.array_equal(got[0, 255, :], 0.0 + (0.0 + (sz * (127.0 - np.arange(128.0))) ** 2))
        assert got[255, 0, 0] == (sx * 255.0) ** 2 + ((sy * 255.0) ** 2 + (sz * 127.0) ** 2)


def test_distance_transform_edt_on_a_hip_tensor_is_scipy(dev):
    rng = np.random.RandomState(4)
    v = (rng.rand(40, 50, 70) < 0.9).astype(np.float32) * 3
    t = torch.from_numpy(v).to(dev)
    got = transform.distance_transform_edt(t)
    assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == v.shape
    assert np.array_equal(got.cpu().numpy(), ndi.distance_transform_edt(v))
    got = transform.distance_transform_edt(t > 0, sampling=(0.75, 0.75, 3.0))
    want = ndi.distance_transform_edt(v, sampling=(0.75, 0.75, 3.0))
    assert np.array_equal(got.cpu().numpy(), want)
    got = transform.distance_transform_edt(t.to(torch.uint8), sampling=(0.75, 0.75, 3.0), squared=True)
    assert np.array_equal(np.sqrt(got.cpu().numpy()), want)
    assert torch.isinf(transform.distance_transform_edt(torch.ones(4, 5, 6, device=dev))).all()   # the one departure


# ------------------------------------------------------------------------------------------------ surface and gather
@pytest.mark.parametrize("shape", [(9, 11, 1), (12, 13, 63), (10, 9, 64), (7, 8, 65), (20, 21, 130), (1, 1, 70), (5, 1, 5)])
def test_surface_is_mask_without_its_erosion(dev, shape):
    rng = np.random.RandomState(sum(shape))
    for mask in (rng.rand(*shape) < 0.8, np.ones(shape, bool), np.zeros(shape, bool)):
        s = distance.surface(packed(mask, dev))
        assert np.array_equal(morphology.unpack(s).cpu().numpy().astype(bool), mask & ~ndi.binary_erosion(mask))
        if shape[2] & 63:                                                      # the bits at z >= Z stay 0
            assert not np.any(s.bits.cpu().numpy().view(np.uint64)[..., -1] >> np.uint64(shape[2] & 63))


def test_surface_ignores_set_tail_bits_of_its_input(dev):
    mask = np.ones((4, 5, 70), bool)
    p = packed(mask, dev)
    p.bits[..., -1] |= -1 << 6                                                 # bits at z >= 70 set by a careless caller
    s = distance.surface(p)
    assert np.array_equal(morphology.unpack(s).cpu().numpy().astype(bool), mask & ~ndi.binary_erosion(mask))
    assert not np.any(s.bits.cpu().numpy().view(np.uint64)[..., -1] >> np.uint64(6))
    assert np.array_equal(distance.edt_squared(p).cpu().numpy(), np.zeros(mask.shape))


@pytest.mark.parametrize("shape", [(33, 35, 70), (16, 16, 64), (3, 5, 1), (40, 40, 130)])
def test_gather_is_numpy_boolean_indexing(dev, shape):
    rng = np.random.RandomState(shape[2])
    sq = rng.rand(*shape)
    query = rng.rand(*shape) < 0.3
    d_sq, q = torch.from_numpy(sq).to(dev), packed(query, dev)
    got = distance.gather(d_sq, q)
    assert got.dtype == torch.float64 and np.array_equal(got.cpu().numpy(), sq[query])
    assert distance.gather(d_sq, packed(np.zeros(shape, bool), dev)).numel() == 0
    n = int(query.sum())
    values, count = distance.gather(d_sq, q, capacity=n + 5)
    assert int(count.item()) == n and np.array_equal(values[:n].cpu().numpy(), sq[query])
    # a buffer that is too small: the count says so and nothing is written at or beyond the capacity
    small = max(n // 2, 1)
    buf = torch.full((small + 64,), -1.0, dtype=torch.float64, device=dev)
    cnt = torch.zeros(1, dtype=torch.int64, device=dev)
    distance._gather_into(d_sq, q, buf[:small], cnt)
    assert int(cnt.item()) == n
    assert np.array_equal(buf[:small].cpu().numpy(), sq[query][:small]) and bool((buf[small:] == -1.0).all())


@pytest.mark.parametrize("shape", [(513, 512, 1), (300, 440, 65)])
def test_gather_scans_more_than_1024_chunk_counts(dev, shape):
    """1026 and 1032 chunks of 256 words (the second shape with a tail word): the one-workgroup scan of the chunk counts
    gives a thread two chunks, and the chunk count is no multiple of its 1024 threads."""
    rng = np.random.RandomState(shape[0])
    sq = rng.rand(*shape)
    query = rng.rand(*shape) < 0.3
    n = int(query.sum())
    values, count = distance.gather(torch.from_numpy(sq).to(dev), packed(query, dev), capacity=n + 5)
    assert int(count.item()) == n
    assert np.array_equal(values[:n].cpu().numpy(), sq[query])


def test_reductions_over_a_gathered_vector(dev):
    rng = np.random.RandomState(9)
    for n, cap in ((1, 1), (5000, 5000), (5000, 9000), (2048, 4096), (70001, 70001)):
        v = rng.rand(cap) * 9.0
        v[:3] = (4.0, 2.25, 0.0)[:cap]                                          # 2.25 sits on the tolerance 1.5
        d_v = torch.from_numpy(v).to(dev)
        count = torch.tensor([n], dtype=torch.int64, device=dev)
        got = distance.reduce(d_v, count, 2.25).cpu().numpy()
        assert got[0] == n and got[1] == v[:n].max() and got[2] == (v[:n] <= 2.25).sum()
        assert got[3] == pytest.approx(np.sqrt(v[:n]).sum(), rel=1e-13)
        assert np.array_equal(distance.reduce(d_v, count, 2.25).cpu().numpy(), got)      # the same bits again
        N.lib.ru3d_set_cu_budget(8)                                            # and under another CU budget
        try:
            with_budget = distance.reduce(d_v, count, 2.25).cpu().numpy()
        finally:
            N.lib.ru3d_set_cu_budget(0)
        assert np.array_equal(with_budget, got)
    over = distance.reduce(d_v, torch.tensor([cap + 10], dtype=torch.int64, device=dev), 2.25).cpu().numpy()
    assert over[0] == cap                                                      # a count above the capacity is clamped
    none = distance.reduce(d_v, torch.zeros(1, dtype=torch.int64, device=dev), 2.25).cpu().numpy()
    assert np.array_equal(none, np.zeros(4))


def test_surface_distances_are_the_brute_force_ones(dev):
    rng = np.random.RandomState(6)
    a, b = rng.rand(12, 13, 70) < 0.7, rng.rand(12, 13, 70) < 0.6
    sa, sb = a & ~ndi.binary_erosion(a), b & ~ndi.binary_erosion(b)
    for spacing in DYADIC + [ODD]:
        got = distance.surface_distances(packed(a, dev), packed(b, dev), spacing)
        assert np.array_equal(got.cpu().numpy(), contract_brute(sb, spacing)[sa])
    got = distance.surface_distances(packed(a, dev), packed(np.zeros_like(b), dev))
    assert got.numel() == sa.sum() and bool(torch.isinf(got).all())


# ------------------------------------------------------------------------------------------------ the metrics
def three_classes(shape=(70, 64, 66)):
    rng = np.random.RandomState(8)
    x, y, z = np.ogrid[:shape[0], :shape[1], :shape[2]]

    def blob(c, r):
        return ((x - c[0]) / r[0]) ** 2 + ((y - c[1]) / r[1]) ** 2 + ((z - c[2]) / r[2]) ** 2 < 1

    label = np.zeros(shape, np.uint8)
    label[blob((34, 30, 32), (26.0, 22.0, 24.0))] = 1
    label[blob((34, 30, 32), (14.0, 12.0, 13.0))] = 2
    label[blob((40, 30, 32), (5.0, 6.0, 4.0))] = 3
    label[:4, :5, 60:] = 3                                                     # a piece that touches the volume's faces
    pred = np.roll(label, (2, -1, 1), axis=(0, 1, 2))
    speckle = rng.rand(*shape) < 0.002
    pred[speckle] = rng.randint(1, 4, size=int(speckle.sum())).astype(np.uint8)
    return pred, label


def assert_same_metrics(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g['hd'] == w['hd'] and g['nsd'] == w['nsd'] and g['hd95'] == w['hd95']
        assert g['assd'] == w['assd'] if math.isinf(w['assd']) else g['assd'] == pytest.approx(w['assd'], rel=1e-12)


def test_evaluate_surface_case_on_hip_operands_equals_the_numpy_route(dev):
    pred, label = three_classes()
    spacing, tolerance = (0.75, 0.75, 3.0), 1.5
    host = {'pred': pred, 'label': label}
    want = trainer.evaluate_surface_case(host, spacing=spacing, tolerance=tolerance)
    d_pred, d_label = torch.from_numpy(pred).to(dev), torch.from_numpy(label).to(dev)
    got = trainer.evaluate_surface_case({'pred': d_pred, 'label': d_label}, spacing=spacing, tolerance=tolerance)
    assert len(got) == 3 and all(0 < m['hd95'] <= m['hd'] < math.inf and 0 < m['nsd'] < 1 for m in got)
    assert_same_metrics(got, want)
    # what hd95 is made of: counts, maxima, tolerance counts and the two order statistics agree exactly
    h_stats = trainer._surface_stats_case(host, spacing, tolerance)
    d_stats = trainer._surface_stats_case({'pred': d_pred, 'label': d_label}, spacing, tolerance)
    for h, d in zip(h_stats, d_stats):
        for key in ('n_ab', 'n_ba', 'max_ab', 'max_ba', 'within_ab', 'within_ba', 'lo', 'hi'):
            assert h[key] == d[key], key
    # the same call again: the same bits
    assert trainer.evaluate_surface_case({'pred': d_pred, 'label': d_label}, spacing=spacing, tolerance=tolerance) == got
    # mixed operands: the numpy one is uploaded
    assert trainer.evaluate_surface_case({'pred': pred, 'label': d_label}, spacing=spacing, tolerance=tolerance) == got
    assert trainer.evaluate_surface_case({'pred': d_pred, 'label': label.astype(np.int64)}, spacing=spacing,
                                         tolerance=tolerance) == got
    # unit spacing by default, and a non-dyadic one within the rounding of a tie
    assert_same_metrics(trainer.evaluate_surface_case({'pred': d_pred, 'label': d_label}), trainer.evaluate_surface_case(host))
    odd_d = trainer.evaluate_surface_case({'pred': d_pred, 'label': d_label}, spacing=ODD)
    odd_h = trainer.evaluate_surface_case(host, spacing=ODD)
    for g, w in zip(odd_d, odd_h):
        assert g['nsd'] == pytest.approx(w['nsd'], abs=1e-3)
        assert all(g[k] == pytest.approx(w[k], rel=1e-12) for k in ('hd', 'hd95', 'assd'))


def test_evaluate_surface_case_empty_mask_rules_on_the_device(dev):
    pred, label = three_classes((40, 44, 70))
    zero = {'hd': 0.0, 'hd95': 0.0, 'assd': 0.0, 'nsd': 1.0}
    none = {'hd': math.inf, 'hd95': math.inf, 'assd': math.inf, 'nsd': 0.0}
    d_label = torch.from_numpy(label).to(dev)
    got = trainer.evaluate_surface_case({'pred': torch.zeros_like(d_label), 'label': d_label})
    assert got == [none] * 3
    assert trainer.evaluate_surface_case({'pred': d_label, 'label': d_label}) == [zero] * 3
    only3 = torch.where(d_label == 3, d_label, torch.zeros_like(d_label))
    got = trainer.evaluate_surface_case({'pred': d_label, 'label': only3})     # classes 1 and 2: the label lacks them
    assert got == [none, none, zero]
    assert trainer.evaluate_surface_case({'pred': d_label, 'label': torch.zeros_like(d_label)}) == []
    got = trainer.evaluate_surface_case({'pred': only3, 'label': d_label})
    assert got == trainer.evaluate_surface_case({'pred': only3.cpu().numpy(), 'label': label})


def test_surface_buffers_grow_when_a_surface_outnumbers_them(dev, monkeypatch):
    pred, label = three_classes((40, 40, 70))
    want = trainer.evaluate_surface_case({'pred': pred, 'label': label}, spacing=(0.75, 0.75, 3.0))
    monkeypatch.setattr(distance, "_INITIAL_CAPACITY", 64)
    monkeypatch.setattr(distance, "_capacity", {})
    got = trainer.evaluate_surface_case({'pred': torch.from_numpy(pred).to(dev), 'label': torch.from_numpy(label).to(dev)},
                                        spacing=(0.75, 0.75, 3.0))
    assert_same_metrics(got, want)
    assert distance._capacity[dev] > 64


def test_evaluate_surface_file_round_trip_uses_the_affines_spacing(dev, tmp_path):
    pred, label = three_classes((40, 44, 70))
    for name, volume, affine in (("label", label, np.diag([0.75, 0.75, 3.0, 1.0])), ("pred", pred, np.eye(4))):
        os.makedirs(tmp_path / name)
        nifti.save(volume, affine, str(tmp_path / name / "case_0.nii.gz"))
    files = (tmp_path / "label" / "case_0.nii.gz", tmp_path / "pred" / "case_0.nii.gz")
    want = trainer.evaluate_surface_case({'pred': pred, 'label': label}, spacing=(0.75, 0.75, 3.0), tolerance=2.0)
    assert trainer.evaluate_surface(*files, tolerance=2.0) == want
    got = trainer.evaluate_surface(*files, tolerance=2.0, device=dev)
    assert_same_metrics(got, want)
    assert got != trainer.evaluate_surface_case({'pred': pred, 'label': label}, tolerance=2.0)
    batch = trainer.batch_evaluate_surface(tmp_path / "label", tmp_path / "pred", tolerance=2.0, device=dev)
    assert batch == [got]


def test_a_prediction_left_in_hbm_goes_in_without_a_download(dev, monkeypatch):
    pred, label = three_classes((40, 44, 70))
    d_pred = torch.from_numpy(pred).to(dev)                                    # what cascade_predict_case(return_device=True) returns
    want = trainer.evaluate_surface_case({'pred': pred, 'label': label}, spacing=(0.75, 0.75, 3.0))
    downloads = []
    real_cpu = torch.Tensor.cpu

    def counting_cpu(self, *args, **kwargs):
        if self.is_cuda:
            downloads.append(self.numel())
        return real_cpu(self, *args, **kwargs)

    monkeypatch.setattr(torch.Tensor, "cpu", counting_cpu)
    got = trainer.evaluate_surface_case({'pred': d_pred, 'label': label}, spacing=(0.75, 0.75, 3.0))
    monkeypatch.undo()
    assert_same_metrics(got, want)
    assert downloads == [10, 10, 10]                                           # one small download per class
