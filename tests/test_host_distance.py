"""CPU-only checks of the distance transform / surface-distance feature: the numpy route of
trainer.evaluate_surface_case on hand-built cases whose answers are written out here and against an all-pairs brute
force, transform.distance_transform_edt on numpy input, a host twin of the device algorithm (Z pass from the packed
words, outward scans with the early exit and the hard bound of csrc/distance.hip) held bit for bit against a brute
force of the contract expression, the argument checks of distance.py and of the C entry points, and the names in the
header, the library, the bindings, the Makefile and the ISA tool."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import scipy.ndimage as ndi
import torch

import _native as N
import distance
import morphology
import nifti
import trainer
import transform

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["ru3d_edt_workspace_bytes", "ru3d_edt_squared", "ru3d_mask_surface", "ru3d_edt_gather_workspace_bytes",
                "ru3d_edt_gather", "ru3d_edt_reduce_workspace_bytes", "ru3d_edt_reduce"]
INF = math.inf


def contract_brute(features, spacing):
    """out[p] = min over the feature voxels f of fl(A + fl(B + C)), A = fl(fl(sx (px - fx))^2): every pair visited."""
    f = np.argwhere(features)
    if not len(f):
        return np.full(features.shape, np.inf)
    p = np.indices(features.shape).reshape(3, -1).T
    a, b, c = ((spacing[k] * (p[:, None, k] - f[None, :, k]).astype(np.float64)) ** 2 for k in range(3))
    return (a + (b + c)).min(axis=1).reshape(features.shape)


def metrics_brute(pred, label, spacing, tolerance):
    """The four metrics of one class from their definitions, through contract_brute."""
    sa, sb = pred & ~ndi.binary_erosion(pred), label & ~ndi.binary_erosion(label)
    d_ab, d_ba = np.sqrt(contract_brute(sb, spacing)[sa]), np.sqrt(contract_brute(sa, spacing)[sb])
    within = (d_ab ** 2 <= tolerance * tolerance).sum() + (d_ba ** 2 <= tolerance * tolerance).sum()
    return {'hd': max(d_ab.max(), d_ba.max()), 'hd95': np.percentile(np.concatenate((d_ab, d_ba)), 95),
            'assd': (d_ab.mean() + d_ba.mean()) / 2, 'nsd': within / (d_ab.size + d_ba.size)}


def boxes(offset):
    pred, label = np.zeros((12, 8, 8), np.uint8), np.zeros((12, 8, 8), np.uint8)
    pred[2:4, 2:4, 2:4] = 1
    label[2 + offset[0]:4 + offset[0], 2 + offset[1]:4 + offset[1], 2 + offset[2]:4 + offset[2]] = 1
    return {'pred': pred, 'label': label}


# ------------------------------------------------------------------------------------------------ hand-built cases
def test_two_boxes_offset_along_x_unit_spacing():
    # 2x2x2 boxes (all surface) three voxels apart along x: from each box four voxels are 2 away and four are 3 away
    got = trainer.evaluate_surface_case(boxes((3, 0, 0)), tolerance=2.0)
    assert got == [{'hd': 3.0, 'hd95': 3.0, 'assd': 2.5, 'nsd': 0.5}]
    assert trainer.evaluate_surface_case(boxes((3, 0, 0)), spacing=(1, 1, 1), tolerance=1.0)[0]['nsd'] == 0.0
    assert trainer.evaluate_surface_case(boxes((3, 0, 0)), tolerance=3.0)[0]['nsd'] == 1.0


def test_two_boxes_anisotropic_spacing_and_a_distance_on_the_tolerance():
    # the same boxes under (0.75, 0.75, 3.0): 1.5 and 2.25 along x; 1.5 sits on the tolerance and counts
    got = trainer.evaluate_surface_case(boxes((3, 0, 0)), spacing=(0.75, 0.75, 3.0), tolerance=1.5)
    assert got == [{'hd': 2.25, 'hd95': 2.25, 'assd': 1.875, 'nsd': 0.5}]
    # two voxels apart along z: the facing layers are 3 apart, the far ones 6
    got = trainer.evaluate_surface_case(boxes((0, 0, 2)), spacing=(0.75, 0.75, 3.0), tolerance=3.0)
    assert got == [{'hd': 6.0, 'hd95': 6.0, 'assd': 4.5, 'nsd': 0.5}]
    # a diagonal offset of single voxels: sqrt(0.75^2 + 1.5^2 + 6^2)
    pred, label = np.zeros((4, 4, 4), np.uint8), np.zeros((4, 4, 4), np.uint8)
    pred[0, 0, 0] = label[1, 2, 2] = 1
    d = math.sqrt(0.5625 + (2.25 + 36.0))
    got = trainer.evaluate_surface_case({'pred': pred, 'label': label}, spacing=(0.75, 0.75, 3.0))
    assert got == [{'hd': d, 'hd95': d, 'assd': d, 'nsd': 0.0}]


def test_identical_empty_and_missing_classes():
    case = boxes((0, 0, 0))
    assert trainer.evaluate_surface_case(case) == [{'hd': 0.0, 'hd95': 0.0, 'assd': 0.0, 'nsd': 1.0}]
    one_empty = {'pred': np.zeros_like(case['label']), 'label': case['label']}
    assert trainer.evaluate_surface_case(one_empty) == [{'hd': INF, 'hd95': INF, 'assd': INF, 'nsd': 0.0}]
    # class 1 is in neither volume (both empty), class 2 only in the label; class 3 of pred is beyond label.max()
    label = np.zeros((6, 6, 6), np.uint8)
    label[1:3, 1:3, 1:3] = 2
    pred = np.zeros((6, 6, 6), np.uint8)
    pred[3:5, 3:5, 3:5] = 3
    got = trainer.evaluate_surface_case({'pred': pred, 'label': label})
    assert got == [{'hd': 0.0, 'hd95': 0.0, 'assd': 0.0, 'nsd': 1.0}, {'hd': INF, 'hd95': INF, 'assd': INF, 'nsd': 0.0}]
    assert trainer.evaluate_surface_case({'pred': pred, 'label': np.zeros_like(label)}) == []
    with pytest.raises(ValueError, match="spacing"):
        trainer.evaluate_surface_case(case, spacing=(1.0, 0.0, 1.0))
    with pytest.raises(ValueError, match="spacing"):
        trainer.evaluate_surface_case(case, spacing=(1.0, 1.0))
    with pytest.raises(ValueError, match="shape"):
        trainer.evaluate_surface_case({'pred': pred, 'label': case['label']})


@pytest.mark.parametrize("spacing", [(1.0, 1.0, 1.0), (0.75, 0.75, 3.0)])
def test_numpy_route_equals_the_all_pairs_brute_force(spacing):
    rng = np.random.RandomState(5)
    x, y, z = np.ogrid[:14, :15, :12]
    label = np.zeros((14, 15, 12), np.uint8)
    label[(x - 6) ** 2 + (y - 7) ** 2 + (z - 5) ** 2 < 22] = 1
    label[(x - 7) ** 2 + (y - 7) ** 2 + (z - 6) ** 2 < 6] = 2
    label[0:3, 0:4, 9:12] = 3                                                  # touches three faces of the volume
    pred = np.roll(label, (1, -1, 1), axis=(0, 1, 2))
    pred[rng.rand(*pred.shape) < 0.02] = 1
    got = trainer.evaluate_surface_case({'pred': pred, 'label': label}, spacing=spacing, tolerance=1.5)
    assert len(got) == 3
    for c, m in enumerate(got, start=1):
        want = metrics_brute(pred == c, label == c, spacing, 1.5)
        assert m['hd'] == want['hd'] and m['nsd'] == want['nsd'], c
        assert m['hd95'] == pytest.approx(want['hd95'], rel=1e-15, abs=0) and m['assd'] == pytest.approx(want['assd'], rel=1e-13)
    # tensors on the host take the numpy route too, and a 2-axis volume is a 1 x Y x Z volume
    again = trainer.evaluate_surface_case({'pred': torch.from_numpy(pred), 'label': label}, spacing=spacing, tolerance=1.5)
    assert again == got
    flat = trainer.evaluate_surface_case({'pred': pred[3], 'label': label[3]}, spacing=spacing[1:], tolerance=1.5)
    assert flat[0]['hd'] == metrics_brute(pred[3:4] == 1, label[3:4] == 1, spacing, 1.5)['hd']


def test_evaluate_surface_reads_the_spacing_of_the_labels_affine(tmp_path, capsys):
    case = boxes((3, 0, 0))
    for name, affine in (("label", np.diag([0.75, 0.75, 3.0, 1.0])), ("pred", np.eye(4))):
        os.makedirs(tmp_path / name)
        nifti.save(case[name], affine, str(tmp_path / name / "case_0.nii.gz"))
    got = trainer.evaluate_surface(tmp_path / "label" / "case_0.nii.gz", tmp_path / "pred" / "case_0.nii.gz", tolerance=1.5)
    assert got == [{'hd': 2.25, 'hd95': 2.25, 'assd': 1.875, 'nsd': 0.5}]
    batch = trainer.batch_evaluate_surface(tmp_path / "label", tmp_path / "pred", tolerance=1.5)
    assert batch == [got]
    out = capsys.readouterr().out
    assert "The mean hd95 of each label:" in out and "label_1: 2.250000" in out


def test_distance_transform_edt_numpy_route_is_scipy():
    rng = np.random.RandomState(1)
    v = (rng.rand(9, 10, 11) < 0.8).astype(np.uint8)
    assert np.array_equal(transform.distance_transform_edt(v), ndi.distance_transform_edt(v))
    want = ndi.distance_transform_edt(v, sampling=(0.75, 0.75, 3.0))
    assert np.array_equal(transform.distance_transform_edt(v, sampling=(0.75, 0.75, 3.0)), want)
    assert np.array_equal(transform.distance_transform_edt(v, (0.75, 0.75, 3.0), squared=True), want * want)


# ------------------------------------------------------------------------------------------------ the algorithm's twin
def twin_nearest(words, Z, z):
    """ed_nearest: the distance in voxels from z to the nearest set bit of a packed row (Python ints as words)."""
    W = len(words)
    tail = ((1 << 64) - 1) & ~((1 << (Z & 63)) - 1) if Z & 63 else 0
    row = [w & ~tail if k == W - 1 else w for k, w in enumerate(words)]
    w, b = z >> 6, z & 63
    best = -1
    m = row[w] & ((1 << (b + 1)) - 1)
    if m:
        best = b - (m.bit_length() - 1)
    else:
        for k in range(w - 1, -1, -1):
            if row[k]:
                best = z - (64 * k + row[k].bit_length() - 1)
                break
    up = -1
    m = row[w] >> b << b
    if m:
        up = (m & -m).bit_length() - 1 - b
    else:
        for k in range(w + 1, W):
            if row[k]:
                up = 64 * k + (row[k] & -row[k]).bit_length() - 1 - z
                break
    return up if up >= 0 and (best < 0 or up < best) else best


def twin_scan(column, s, steps):
    """ed_scan along one column: outward on both sides, stop once fl(fl(s d)^2) alone reaches the best so far; the
    number of trips is recorded and may never exceed the hard bound max(l, L - 1 - l)."""
    L, out = len(column), np.empty(len(column))
    for l in range(L):
        best, reach, trips = column[l], max(l, L - 1 - l), 0
        for d in range(1, reach + 1):
            t = np.float64(s) * np.float64(d)
            a = t * t
            if a >= best:
                break
            trips += 1
            lo = column[l - d] if l - d >= 0 else np.inf
            hi = column[l + d] if l + d < L else np.inf
            best = min(best, a + min(lo, hi))
        assert trips <= reach < L
        steps.append(trips)
        out[l] = best
    return out


def twin_edt(features, spacing):
    X, Y, Z = features.shape
    W = (Z + 63) // 64
    steps, out = [], np.empty(features.shape)
    for x in range(X):
        for y in range(Y):
            bits = features[x, y]
            words = [sum(1 << b for b in range(min(64, Z - 64 * k)) if bits[64 * k + b]) for k in range(W)]
            for z in range(Z):
                dz = twin_nearest(words, Z, z)
                t = np.float64(spacing[2]) * np.float64(dz)
                out[x, y, z] = t * t if dz >= 0 else np.inf
    for x in range(X):
        for z in range(Z):
            out[x, :, z] = twin_scan(out[x, :, z].copy(), spacing[1], steps)
    for y in range(Y):
        for z in range(Z):
            out[:, y, z] = twin_scan(out[:, y, z].copy(), spacing[0], steps)
    return out, steps


@pytest.mark.parametrize("spacing", [(1.0, 1.0, 1.0), (0.75, 0.75, 3.0), (0.7, 0.83, 3.1)])
def test_twin_of_the_device_algorithm_equals_the_contract_bit_for_bit(spacing):
    rng = np.random.RandomState(11)
    cases = [rng.rand(5, 6, 70) < 0.03, rng.rand(4, 5, 9) < 0.5, np.zeros((3, 4, 65), bool), np.zeros((6, 5, 4), bool)]
    cases[2][0, 0, 64] = True                                                  # one feature, in the second word
    cases[3][5, :, :] = rng.rand(5, 4) < 0.5                                   # features on one face only
    for features in cases:
        got, steps = twin_edt(features, spacing)
        assert np.array_equal(got, contract_brute(features, spacing)), features.shape
        assert max(steps) < max(features.shape)
    got, steps = twin_edt(np.zeros((3, 4, 5), bool), spacing)                  # no feature: +inf, every scan runs to its bound
    assert np.isinf(got).all() and max(steps) == 3


# ------------------------------------------------------------------------------------------------ entry points
def test_header_library_and_bindings_name_the_distance_entry_points():
    text = open(os.path.join(ROOT, "include", "ru3d.h")).read()
    raw = ctypes.CDLL(N.LIB_PATH)
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert hasattr(raw, name), name
        assert name in N.SIGNATURES, name
    csrc = os.path.join(ROOT, "3d-unet-renal-anatomy-extraction_amd", "csrc")
    makefile = open(os.path.join(csrc, "Makefile")).read()
    assert makefile.count("distance.hip") == 1                                 # once: no 16-bit twin
    assert "distance.hip" in open(os.path.join(ROOT, "tools", "isa_check.py")).read()
    assert os.path.exists(os.path.join(ROOT, "profiles", "distance_isa_check.txt"))
    assert N.lib.ru3d_version() == 201
    assert N.EDT_MAX_AXIS == int(re.search(r"#define RU3D_EDT_MAX_AXIS (\d+)", text).group(1)) >= 2048


def test_c_argument_checks_answer_before_any_launch():
    lib = N.lib
    fake, other = ctypes.c_void_p(4096), ctypes.c_void_p(8192)                  # never dereferenced on these paths
    ok = (ctypes.c_double * 3)(0.75, 0.75, 3.0)

    def failed(rc, word):
        return rc < 0 and word in lib.ru3d_last_error()

    assert lib.ru3d_edt_workspace_bytes(512, 512, 256) >= 4
    assert lib.ru3d_edt_workspace_bytes(2048, 1024, 1024) == 0 and lib.ru3d_edt_workspace_bytes(4, 0, 4) == 0
    assert lib.ru3d_edt_workspace_bytes(N.EDT_MAX_AXIS + 1, 4, 4) == 0 and lib.ru3d_edt_workspace_bytes(4, 4, 100000) > 0
    ws = lib.ru3d_edt_workspace_bytes(8, 8, 8)
    assert failed(lib.ru3d_edt_squared(None, 8, 8, 8, ok, fake, other, ws, None), b"null")
    assert failed(lib.ru3d_edt_squared(fake, 8, 8, 8, None, fake, other, ws, None), b"null")
    assert failed(lib.ru3d_edt_squared(fake, 8, 8, 8, ok, None, other, ws, None), b"null")
    assert failed(lib.ru3d_edt_squared(fake, 8, 8, 8, ok, fake, None, ws, None), b"null")
    assert failed(lib.ru3d_edt_squared(fake, 8, 0, 8, ok, fake, other, ws, None), b"not supported")
    assert failed(lib.ru3d_edt_squared(fake, -8, 8, 8, ok, fake, other, ws, None), b"not supported")
    assert failed(lib.ru3d_edt_squared(fake, 2048, 1024, 1024, ok, fake, other, ws, None), b"2^31")
    assert failed(lib.ru3d_edt_squared(fake, N.EDT_MAX_AXIS + 1, 8, 8, ok, fake, other, ws, None), b"limit of 4096")
    assert failed(lib.ru3d_edt_squared(fake, 8, N.EDT_MAX_AXIS + 1, 8, ok, fake, other, ws, None), b"limit of 4096")
    for bad in (0.0, -1.0, math.inf, math.nan):
        for axis in range(3):
            spacing = (ctypes.c_double * 3)(1.0, 1.0, 1.0)
            spacing[axis] = bad
            assert failed(lib.ru3d_edt_squared(fake, 8, 8, 8, spacing, fake, other, ws, None), b"spacing[%d]" % axis)
    assert failed(lib.ru3d_edt_squared(fake, 8, 8, 8, ok, fake, other, ws - 1, None), b"workspace")
    assert failed(lib.ru3d_mask_surface(fake, fake, 8, 8, 8, None), b"in-place")
    assert failed(lib.ru3d_mask_surface(None, fake, 8, 8, 8, None), b"null")
    assert failed(lib.ru3d_mask_surface(fake, other, 8, 8, 0, None), b"not supported")
    assert lib.ru3d_edt_gather_workspace_bytes(512, 512, 256) >= 512 * 512 * 4 // 256 * 4
    assert lib.ru3d_edt_gather_workspace_bytes(0, 8, 8) == 0
    gws = lib.ru3d_edt_gather_workspace_bytes(8, 8, 8)
    assert failed(lib.ru3d_edt_gather(fake, None, 8, 8, 8, fake, 10, fake, other, gws, None), b"null")
    assert failed(lib.ru3d_edt_gather(None, fake, 8, 8, 8, fake, 10, fake, other, gws, None), b"null")
    assert failed(lib.ru3d_edt_gather(fake, fake, 8, 8, 8, fake, 10, None, other, gws, None), b"null")
    assert failed(lib.ru3d_edt_gather(fake, fake, 8, 8, 8, fake, 0, fake, other, gws, None), b"capacity")
    assert failed(lib.ru3d_edt_gather(fake, fake, 8, 8, 8, fake, 10, fake, other, gws - 1, None), b"workspace")
    assert failed(lib.ru3d_edt_gather(fake, fake, 1 << 16, 1 << 15, 1, fake, 10, fake, other, gws, None), b"2^31")
    assert lib.ru3d_edt_reduce_workspace_bytes(0) == 0 and lib.ru3d_edt_reduce_workspace_bytes(2049) >= 2 * 3 * 8
    rws = lib.ru3d_edt_reduce_workspace_bytes(100)
    assert failed(lib.ru3d_edt_reduce(fake, fake, 0, 1.0, fake, other, rws, None), b"capacity")
    assert failed(lib.ru3d_edt_reduce(None, fake, 100, 1.0, fake, other, rws, None), b"null")
    assert failed(lib.ru3d_edt_reduce(fake, None, 100, 1.0, fake, other, rws, None), b"null")
    assert failed(lib.ru3d_edt_reduce(fake, fake, 100, -1.0, fake, other, rws, None), b"tolerance")
    assert failed(lib.ru3d_edt_reduce(fake, fake, 100, math.nan, fake, other, rws, None), b"tolerance")
    assert failed(lib.ru3d_edt_reduce(fake, fake, 100, 1.0, fake, other, rws - 1, None), b"workspace")


def test_distance_module_refuses_what_it_does_not_do():
    def packed(shape):
        shape3 = (1,) * (3 - len(shape)) + tuple(shape)
        return morphology.PackedMask(torch.zeros((shape3[0], shape3[1], (shape3[2] + 63) // 64), dtype=torch.int64), shape)

    with pytest.raises(ValueError, match="PackedMask"):
        distance.edt_squared(np.zeros((4, 4, 4), bool))
    with pytest.raises(ValueError, match="limit of %d" % N.EDT_MAX_AXIS):
        distance.edt_squared(packed((N.EDT_MAX_AXIS + 1, 2, 2)))
    with pytest.raises(ValueError, match="sampling"):
        distance.edt_squared(packed((4, 4, 4)), sampling=(1.0, -1.0, 1.0))
    with pytest.raises(ValueError, match="sampling"):
        distance.edt_squared(packed((4, 4, 4)), sampling=(1.0, 1.0))
    for call in (lambda: distance.edt_squared(packed((4, 4, 4))), lambda: distance.surface(packed((4, 4, 4))),
                 lambda: distance.surface_distances(packed((4, 4, 4)), packed((4, 4, 4)))):
        with pytest.raises(N.Ru3dError, match="no CPU fallback"):                # device only, like morphology.py
            call()
    with pytest.raises(ValueError, match="PackedMask"):
        distance.surface(torch.zeros(4, 4, 4))
    with pytest.raises(ValueError, match="float64"):
        distance.gather(torch.zeros(4, 4, 4), packed((4, 4, 4)))
    with pytest.raises(N.Ru3dError, match="no CPU fallback"):
        transform.distance_transform_edt(torch.zeros(4, 4, 4))
