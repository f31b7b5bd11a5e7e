"""The mesh kernels (csrc/mesh.hip) against the numpy route of transform.extract_mesh, which restates the contract of
include/ru3d.h: corners, faces and neighbours equal, smoothed positions equal with ==, the measures to 1e-12 and
with the same bits in every run and under every CU budget, capacities respected, the case-level driver on HIP operands
and on the result of a cascade prediction that stays in HBM.  `-m gpu` only."""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no HIP device", allow_module_level=True)

import _native as N  # noqa: E402
from _native import check, ptr, stream  # noqa: E402
import mesh  # noqa: E402
import morphology  # noqa: E402
import network  # noqa: E402
import trainer as T  # noqa: E402
import transform  # noqa: E402

DEV = torch.device("cuda:0")


def random_mask(shape, seed, density=0.35):
    rng = np.random.RandomState(seed)
    m = rng.rand(*shape) < density
    m[0, 0, 0] = m[-1, -1, -1] = True                                       # voxels on the volume's border
    return m


def phantom(shape):
    """Two ellipsoids with a nested third, as labels 1 (shell), 2 (inside the first) and 1 again for the second."""
    x, y, z = np.ogrid[:shape[0], :shape[1], :shape[2]]

    def blob(c, r):
        return ((x - c[0]) / r[0]) ** 2 + ((y - c[1]) / r[1]) ** 2 + ((z - c[2]) / r[2]) ** 2 < 1

    s = np.array(shape, dtype=np.float64)
    v = np.zeros(shape, np.uint8)
    v[blob(s * (0.3, 0.5, 0.5), s * (0.17, 0.22, 0.28))] = 1
    v[blob(s * (0.3, 0.5, 0.5), s * (0.1, 0.13, 0.17))] = 2
    v[blob(s * (0.72, 0.5, 0.45), s * (0.16, 0.2, 0.27))] = 1
    return v


def same_mesh(dev, host):
    assert dev.shape == host.shape
    for name in ("corners", "faces", "neighbours"):
        got, want = getattr(dev, name), torch.from_numpy(getattr(host, name))
        assert got.dtype == torch.int32 and got.is_cuda and tuple(got.shape) == tuple(want.shape), name
        assert torch.equal(got.cpu(), want), name
    assert np.array_equal(dev.vertices.cpu().numpy(), host.vertices)


SHAPES = [(5, 6, 1), (4, 5, 63), (6, 3, 64), (3, 7, 65), (9, 4, 130), (1, 1, 7), (17, 1, 3)]


@pytest.mark.parametrize("shape", SHAPES)
def test_extract_equals_the_numpy_route_on_random_masks(shape):
    m = random_mask(shape, sum(shape))
    host = transform.extract_mesh(m, 0)
    dev = transform.extract_mesh(torch.from_numpy(m).to(DEV), 0)
    same_mesh(dev, host)
    assert mesh.count(torch.from_numpy(m).to(DEV)) == (len(host.corners), len(host.faces) // 2)
    packed = morphology.pack(torch.from_numpy(m.astype(np.uint8)).to(DEV))
    same_mesh(mesh.extract(packed), host)                                  # PackedMask and volume inputs agree
    area, volume = mesh.measure(dev.vertices, dev.faces).tolist()
    assert volume == float(m.sum()) and area == float(len(host.faces) // 2)


def test_extract_scans_more_than_1024_chunk_counts():
    """(513, 512, 1): 1031 chunks of corner words and 1026 of mask words, so both lists of the one-workgroup-per-list scan
    give a thread two chunks and neither count is a multiple of its 1024 threads.  Sparse, so the numpy route stays quick."""
    shape = (513, 512, 1)
    m = random_mask(shape, sum(shape), density=0.02)
    host = transform.extract_mesh(m, 0)
    dev = transform.extract_mesh(torch.from_numpy(m).to(DEV), 0)
    same_mesh(dev, host)
    assert mesh.count(torch.from_numpy(m).to(DEV)) == (len(host.corners), len(host.faces) // 2)
    packed = morphology.pack(torch.from_numpy(m.astype(np.uint8)).to(DEV))
    same_mesh(mesh.extract(packed), host)
    area, volume = mesh.measure(dev.vertices, dev.faces).tolist()
    assert volume == float(m.sum()) and area == float(len(host.faces) // 2)


def test_extract_of_empty_full_and_single_voxel_volumes():
    empty = transform.extract_mesh(torch.zeros((7, 5, 70), dtype=torch.uint8, device=DEV))
    assert tuple(empty.corners.shape) == (0, 3) and tuple(empty.faces.shape) == (0, 3)
    assert tuple(empty.neighbours.shape) == (0, 6) and tuple(empty.vertices.shape) == (0, 3)
    assert mesh.measure(empty.vertices, empty.faces).tolist() == [0.0, 0.0]
    full = np.ones((6, 5, 64), bool)
    same_mesh(transform.extract_mesh(torch.from_numpy(full).to(DEV), 0), transform.extract_mesh(full, 0))
    one = transform.extract_mesh(torch.ones((1, 1, 1), dtype=torch.bool, device=DEV), 0)
    same_mesh(one, transform.extract_mesh(np.ones((1, 1, 1), bool), 0))
    assert len(one.corners) == 8 and len(one.faces) == 12
    assert mesh.measure(one.vertices, one.faces).tolist() == [6.0, 1.0]
    line = np.ones(70, bool)                                                # a volume of one axis keeps its shape
    same_mesh(transform.extract_mesh(torch.from_numpy(line).to(DEV), 0), transform.extract_mesh(line, 0))


def test_extract_smooth_and_measure_on_the_phantom():
    v = phantom((256, 256, 160))
    for value in (1, 2):
        host = transform.extract_mesh(v == value, 0)
        packed = morphology.pack(torch.from_numpy(v).to(DEV), 'eq', value)
        dev = mesh.extract(packed)
        same_mesh(dev, host)
        assert len(host.corners) > 10000
        area, volume = mesh.measure(dev.vertices, dev.faces).tolist()
        assert volume == float((v == value).sum()) and area == float(len(host.faces) // 2)
        smooth_host = transform.extract_mesh(v == value, 10)
        smooth_dev = mesh.smooth(dev, 10)
        assert np.array_equal(smooth_dev.vertices.cpu().numpy(), smooth_host.vertices)
        want = transform._measure_mesh_numpy(smooth_host.vertices, smooth_host.faces)
        got = mesh.measure(smooth_dev.vertices, smooth_dev.faces).tolist()
        assert got == pytest.approx(want, rel=1e-12)
        assert got[0] < area and abs(got[1] - volume) < 0.01 * volume


def test_capacities_are_respected_and_counts_stay_true():
    m = random_mask((9, 8, 70), 5)
    host = transform.extract_mesh(m, 0)
    V, Q = len(host.corners), len(host.faces) // 2
    packed = morphology.pack(torch.from_numpy(m).to(DEV))
    X, Y, Z = packed.shape3
    ws = N.workspace(N.lib.ru3d_mesh_workspace_bytes(X, Y, Z), DEV)
    for vcap, qcap in ((V // 2, Q // 3), (V, Q), (0, Q // 2), (V // 2, 0), (V + 5, Q + 5)):
        guard = 64
        corners = torch.full((vcap + guard, 3), -7, dtype=torch.int32, device=DEV)
        neighbours = torch.full((vcap + guard, 6), -7, dtype=torch.int32, device=DEV)
        faces = torch.full((2 * (qcap + guard), 3), -7, dtype=torch.int32, device=DEV)
        counts = torch.zeros(2, dtype=torch.int64, device=DEV)
        N.note_device(DEV)
        check(N.lib.ru3d_mesh_emit(ptr(packed.bits), X, Y, Z, ptr(corners), ptr(neighbours), vcap, ptr(faces), qcap,
                                   ptr(counts), ptr(ws), ws.numel(), stream()), "mesh_emit")
        assert counts.tolist() == [V, Q]
        nv, nq = min(V, vcap), min(Q, qcap)
        assert np.array_equal(corners[:nv].cpu().numpy(), host.corners[:nv])
        assert np.array_equal(neighbours[:nv].cpu().numpy(), host.neighbours[:nv])
        assert np.array_equal(faces[:2 * nq].cpu().numpy(), host.faces[:2 * nq])
        assert (corners[nv:] == -7).all() and (neighbours[nv:] == -7).all() and (faces[2 * nq:] == -7).all()


def test_smoothing_equals_the_numpy_route_bit_for_bit():
    g = np.indices((32, 32, 32)) + 0.5 - 16
    ball = (g ** 2).sum(axis=0) <= 144
    dev = mesh.extract(morphology.pack(torch.from_numpy(ball).to(DEV)))
    assert mesh.smooth(dev, 0).vertices.data_ptr() == dev.vertices.data_ptr()
    for iterations in (1, 10):
        host = transform.extract_mesh(ball, iterations)
        got = mesh.smooth(dev, iterations)
        assert np.array_equal(got.vertices.cpu().numpy(), host.vertices), iterations
        assert got.faces is dev.faces and got.neighbours is dev.neighbours
    other = transform.extract_mesh(random_mask((7, 9, 66), 3), 3, lam=0.33, mu=-0.34)
    got = transform.extract_mesh(torch.from_numpy(random_mask((7, 9, 66), 3)).to(DEV), 3, lam=0.33, mu=-0.34)
    assert np.array_equal(got.vertices.cpu().numpy(), other.vertices)
    area, volume = mesh.measure(mesh.smooth(dev, 10).vertices, dev.faces).tolist()
    assert abs(area - 4 * math.pi * 144) < 0.06 * 4 * math.pi * 144 and abs(volume - 7208) < 72.08


def test_measures_have_the_same_bits_in_every_run_and_under_every_cu_budget():
    v = phantom((96, 96, 80))
    m = mesh.smooth(mesh.extract(morphology.pack(torch.from_numpy(v).to(DEV), 'eq', 1)), 4)
    assert len(m.faces) > 3 * 2048                                          # several partials
    want = transform._measure_mesh_numpy(m.vertices.cpu().numpy(), m.faces.cpu().numpy())
    first = mesh.measure(m.vertices, m.faces).tolist()
    assert first == pytest.approx(want, rel=1e-12)
    assert mesh.measure(m.vertices, m.faces).tolist() == first
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    try:
        for budget in (32, cus):
            assert N.lib.ru3d_set_cu_budget(budget) == 0
            assert mesh.measure(m.vertices, m.faces).tolist() == first, budget
            again = mesh.smooth(mesh.extract(morphology.pack(torch.from_numpy(v).to(DEV), 'eq', 1)), 4)
            assert torch.equal(again.vertices, m.vertices) and torch.equal(again.faces, m.faces), budget
    finally:
        N.lib.ru3d_set_cu_budget(0)


def rotated_affine():
    c, s = math.cos(0.4), math.sin(0.4)
    a = np.eye(4)
    a[:3, :3] = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]) @ np.diag([0.75, 0.8, 3.0])
    a[:3, 3] = (-120.5, 33.25, 801.0)
    return a


@pytest.mark.parametrize("flip", [False, True])
def test_extract_mesh_case_on_hip_operands_equals_the_numpy_route(flip):
    v = phantom((48, 40, 70))
    affine = rotated_affine()
    if flip:
        affine[:3, 0] *= -1
    case = {'pred': v, 'affine': affine}
    labels = [(1, 2), 2]
    host = T.extract_mesh_case(case, labels)
    dev = T.extract_mesh_case({'pred': torch.from_numpy(v).to(DEV), 'affine': affine}, labels)
    kept = T.extract_mesh_case({'pred': torch.from_numpy(v).to(DEV), 'affine': affine}, labels, return_device=True)
    assert [r['label'] for r in dev] == [(1, 2), 2] == [r['label'] for r in host]
    for h, d, k in zip(host, dev, kept):
        assert isinstance(d['vertices'], np.ndarray) and d['vertices'].dtype == np.float64
        assert np.array_equal(d['faces'], h['faces']) and d['faces'].dtype == np.int32
        assert np.abs(d['vertices'] - h['vertices']).max() <= 1e-9
        assert d['area'] == pytest.approx(h['area'], rel=1e-12) and d['volume'] == pytest.approx(h['volume'], rel=1e-12)
        assert d['volume'] > 0 and abs(d['volume'] - np.isin(v, h['label']).sum() * 1.8) < 0.02 * d['volume']
        assert k['vertices'].is_cuda and k['faces'].is_cuda and torch.equal(k['faces'].cpu(), torch.from_numpy(d['faces']))
        assert k['area'] == d['area'] and k['volume'] == d['volume']
    every = T.extract_mesh_case({'pred': torch.from_numpy(v).to(DEV)}, smooth_iterations=0)       # labels 1 .. max
    assert [r['label'] for r in every] == [1, 2]
    assert [r['volume'] for r in every] == [float((v == 1).sum()), float((v == 2).sum())]


def test_a_cascade_prediction_that_stays_in_hbm_becomes_meshes_without_a_host_copy(golden_dir):
    z = np.load(os.path.join(golden_dir, "g9_cascade.npz"))
    coarse = network.ResUnet3D(num_pool=2, num_features=4, in_channels=1, out_channels=1)
    detail = network.ResUnet3D(num_pool=2, num_features=4, in_channels=1, out_channels=3)
    coarse.load_state_dict({k[len("coarse/w/"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("coarse/w/")})
    detail.load_state_dict({k[len("detail/w/"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("detail/w/")})
    stats = dict(zip(("mean", "std", "pct_00_5", "pct_99_5"), (float(v) for v in z["stats"])))
    case = {"case_id": "g9", "image": z["image"], "affine": z["affine"]}
    out = T.cascade_predict_case(case, coarse.to(DEV).eval(), tuple(z["params"][0]), stats,
                                 tuple(int(v) for v in z["patches"][0]), detail.to(DEV).eval(), tuple(z["params"][1]),
                                 stats, tuple(int(v) for v in z["patches"][1]), step_per_patch=int(z["scalars"][0]),
                                 region_threshold=int(z["scalars"][1]), crop_padding=int(z["scalars"][2]), verbose=False,
                                 on_device=True, return_device=True)
    assert torch.is_tensor(out["pred"]) and out["pred"].is_cuda and out["pred"].dtype == torch.uint8
    dev = T.extract_mesh_case(out, smooth_iterations=4)
    pred = out["pred"].cpu().numpy()
    assert pred.max() >= 1 and len(dev) == int(pred.max())
    host = T.extract_mesh_case({"pred": pred, "affine": out["affine"]}, smooth_iterations=4)
    for h, d in zip(host, dev):
        assert np.array_equal(d['faces'], h['faces']) and np.abs(d['vertices'] - h['vertices']).max() <= 1e-9
        assert d['volume'] == pytest.approx(h['volume'], rel=1e-12)
    assert sum(len(d['faces']) for d in dev) > 0
