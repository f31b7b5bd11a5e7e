"""GPU checks of csrc/territory.hip and what is built on it: territory.nearest (index and squared distance) with == against
the numpy twin that defines it and against distance.edt_squared - word boundaries, degenerate tiles and long scans, three
spacings, sparse, dense, one-face and empty site masks, a capped grid - territory.assign and territory.tally against their
twins on both tally paths, repeatability, the memory contract (inputs, guard regions, short workspaces, what only the
device can see), and transform.nearest_feature and the trainer's territory drivers on HIP operands against the host
route."""
import numpy as np
import pytest
import scipy.ndimage as ndi
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no HIP device", allow_module_level=True)

import ctypes  # noqa: E402

import _native as N  # noqa: E402
import distance  # noqa: E402
import morphology  # noqa: E402
import nifti  # noqa: E402
import territory  # noqa: E402
import trainer  # noqa: E402
import transform  # noqa: E402
from utils import json_load  # noqa: E402
from test_host_skeleton import blob, tree_case  # noqa: E402
from test_host_skeleton_graph import same  # noqa: E402

SPACINGS = [(1.0, 1.0, 1.0), (0.75, 0.5, 3.0), (0.7, 0.9, 1.3)]


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def packed(volume, dev):
    return morphology.pack(torch.from_numpy(np.array(volume)).to(dev))      # a copy: shared fixtures are read-only


def on(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def check_nearest(volume, dev, spacing=None):
    """territory.nearest of `volume` against the twin and against distance.edt_squared with ==; the bits stay."""
    sites = packed(volume, dev)
    before = sites.bits.clone()
    index, sq = territory.nearest(sites, spacing)
    volume3 = volume.reshape((1,) * (3 - volume.ndim) + volume.shape)
    spacing3 = (1.0,) * 3 if spacing is None else (1.0,) * (3 - len(spacing)) + tuple(spacing)
    want_index, want_sq = transform._nearest_site_numpy(volume3, spacing3)
    assert index.dtype == torch.int32 and sq.dtype == torch.float64 and tuple(index.shape) == volume.shape == tuple(sq.shape)
    assert torch.equal(sites.bits, before)
    assert torch.equal(sq.cpu(), torch.from_numpy(want_sq.reshape(volume.shape)))
    assert torch.equal(index.cpu(), torch.from_numpy(want_index.reshape(volume.shape)))
    assert torch.equal(sq, distance.edt_squared(sites, spacing))
    only, none = territory.nearest(sites, spacing, return_sq=False)
    assert none is None and torch.equal(only, index)
    return index, sq


@pytest.mark.parametrize("Z", [1, 2, 63, 64, 65, 130])
def test_nearest_across_word_boundaries(dev, Z):
    volume = np.random.RandomState(Z).rand(7, 9, Z) < 0.04
    volume[3, 4, Z // 2] = True
    for spacing in SPACINGS:
        check_nearest(volume, dev, spacing)


@pytest.mark.parametrize("shape", [(1, 1, 300), (1, 300, 1), (300, 1, 1), (33, 40, 70)])
def test_nearest_on_degenerate_tiles_and_long_scans(dev, shape):
    volume = np.zeros(shape, dtype=bool)
    volume.reshape(-1)[[3, volume.size // 2 + 5]] = True                    # two sites: scans of more than a hundred steps
    for spacing in SPACINGS:
        check_nearest(volume, dev, spacing)
    check_nearest(np.random.RandomState(1).rand(*shape) < 0.02, dev, SPACINGS[1])


def test_nearest_sparse_dense_face_and_empty(dev):
    shape = (12, 20, 70)
    one = np.zeros(shape, dtype=bool)
    one[11, 0, 64] = True
    face = np.zeros(shape, dtype=bool)
    face[0] = np.random.RandomState(2).rand(20, 70) < 0.3
    for volume in (one, blob(3, shape), face):
        for spacing in SPACINGS:
            check_nearest(volume, dev, spacing)
    index, sq = check_nearest(np.zeros(shape, dtype=bool), dev, SPACINGS[1])
    assert bool((index == -1).all()) and bool(torch.isinf(sq).all())
    plane = np.zeros((9, 12), dtype=bool)                                   # fewer axes
    plane[4, 1] = plane[2, 10] = True
    check_nearest(plane, dev, (0.5, 2.0))
    check_nearest(np.array([0, 1, 0, 0, 0, 1, 0], dtype=bool), dev)


def check_assign_tally(dev, sites, site_ids, K, region=None, other=None, num_other=0):
    index_np, _ = transform._nearest_site_numpy(sites)
    want_labels = transform._site_assign_numpy(sites, site_ids, index_np, region)
    want_table = transform._territory_tally_numpy(want_labels, K, other, num_other, region)
    s, r = packed(sites, dev), None if region is None else packed(region, dev)
    index, _ = territory.nearest(s)
    ids, o = on(dev, site_ids), None if other is None else on(dev, other)
    kept = [t.clone() for t in (s.bits, index, ids)] + ([r.bits.clone()] if r is not None else []) + ([o.clone()] if o is not None else [])
    labels = territory.assign(s, ids, index, r)
    table = territory.tally(labels, K, o, num_other, r)
    assert labels.dtype == torch.int32 and torch.equal(labels.cpu(), torch.from_numpy(want_labels))
    assert table.dtype == torch.int64 and torch.equal(table.cpu(), torch.from_numpy(want_table))
    now = [s.bits, index, ids] + ([r.bits] if r is not None else []) + ([o] if o is not None else [])
    assert all(torch.equal(a, b) for a, b in zip(kept, now))                # the inputs are left alone
    assert int(want_table.sum()) == (sites.size if region is None else int(region.sum()))
    return want_table


def test_assign_and_tally_against_the_twins(dev):
    rng = np.random.RandomState(4)
    shape = (9, 11, 70)
    sites = rng.rand(*shape) < 0.02
    n = int(sites.sum())
    site_ids = rng.randint(1, 7, n).astype(np.int32)
    region = ndi.binary_dilation(rng.rand(*shape) < 0.01, iterations=3)
    other = rng.randint(0, 5, shape).astype(np.uint8)
    assert (sites & ~region).any()                                          # sites outside the region still attract
    check_assign_tally(dev, sites, site_ids, 6)
    check_assign_tally(dev, sites, site_ids, 6, region)
    check_assign_tally(dev, sites, site_ids, 6, None, other, 4)
    table = check_assign_tally(dev, sites, site_ids, 6, region, other, 2)   # 3 and 4 land in the last column
    assert table[:, 2].sum() == int((region & (other >= 2)).sum()) > 0
    check_assign_tally(dev, sites, site_ids, 9, region, other, 0)           # one column, rows without a voxel
    empty = check_assign_tally(dev, sites, site_ids, 6, np.zeros(shape, dtype=bool), other, 2)
    assert int(empty.sum()) == 0
    nothing = check_assign_tally(dev, np.zeros(shape, dtype=bool), np.zeros(0, np.int32), 3, region)
    assert nothing[0, 0] == int(region.sum())                               # no site: every region voxel in row 0


def test_tally_beyond_the_lds_table(dev):
    rng = np.random.RandomState(5)
    shape = (40, 40, 70)
    sites = rng.rand(*shape) < 0.05
    n = int(sites.sum())
    assert n >= 5000
    site_ids = rng.permutation(n).astype(np.int32) + 1                      # K = n ids: (K + 1) * 2 cells are beyond LDS
    region = ndi.binary_dilation(rng.rand(*shape) < 0.002, iterations=6)
    other = (rng.rand(*shape) < 0.3).astype(np.uint8)
    table = check_assign_tally(dev, sites, site_ids, n, region, other, 1)
    assert table.shape == (n + 1, 2) and (table.sum(axis=1) > 0).sum() > 1000
    check_assign_tally(dev, sites, site_ids, n)


def test_capped_grid(dev):
    """(136, 128, 64): 544 tiles in the ZY pass and 512 in the X pass, 4352 blocks in the voxel loops.  Under a budget of 8
    CUs the grids are 24 and 64 workgroups, so every persistent loop makes many trips."""
    shape = (136, 128, 64)
    volume = blob(11, shape) & (np.random.RandomState(6).rand(*shape) < 0.05)
    assert volume.any()
    want_index, want_sq = transform._nearest_site_numpy(volume, SPACINGS[1])
    n = int(volume.sum())
    site_ids = (np.arange(n) % 11 + 1).astype(np.int32)
    region = blob(12, shape)
    other = (np.indices(shape).sum(axis=0) % 3).astype(np.uint8)
    want_labels = transform._site_assign_numpy(volume, site_ids, want_index, region)
    want_table = transform._territory_tally_numpy(want_labels, 11, other, 2, region)

    def run():
        sites, r = packed(volume, dev), packed(region, dev)
        index, sq = territory.nearest(sites, SPACINGS[1])
        labels = territory.assign(sites, on(dev, site_ids), index, r)
        return index, sq, labels, territory.tally(labels, 11, on(dev, other), 2, r)

    free = run()
    try:
        assert N.lib.ru3d_set_cu_budget(8) == 0
        capped = run()
    finally:
        N.lib.ru3d_set_cu_budget(0)
    assert N.lib.ru3d_get_cu_budget() == torch.cuda.get_device_properties(dev).multi_processor_count
    for got in (free, capped):
        for g, w in zip(got, (want_index, want_sq, want_labels, want_table)):
            assert torch.equal(g.cpu(), torch.from_numpy(w))


def test_repeatable(dev):
    volume = blob(7, (17, 19, 67))
    sites = packed(transform._skeleton_numpy(volume)[0], dev)
    region = packed(volume, dev)
    n = int(morphology.unpack(sites).sum().item())
    ids = torch.arange(1, n + 1, dtype=torch.int32, device=dev)
    runs = []
    for _ in range(2):
        index, sq = territory.nearest(sites, SPACINGS[2])
        labels = territory.assign(sites, ids, index, region)
        runs.append((index, sq, labels, territory.tally(labels, n, None, 0, region)))
    assert all(torch.equal(a, b) for a, b in zip(*runs))


def guarded(n, dtype, fill, dev, pad=64):
    """(buffer, view of n elements in its middle, check that everything around the view is still `fill`)."""
    buf = torch.full((n + 2 * pad,), fill, dtype=dtype, device=dev)
    return buf, buf[pad:pad + n], lambda: bool((buf[:pad] == fill).all()) and bool((buf[pad + n:] == fill).all())


def test_memory_contract(dev):
    volume = blob(7, (17, 19, 67))
    sites_np = transform._skeleton_numpy(volume)[0]
    sites, region = packed(sites_np, dev), packed(volume, dev)
    X, Y, Z = sites.shape3
    n, voxels = int(sites_np.sum()), X * Y * Z
    stream = torch.cuda.current_stream(dev).cuda_stream
    spacing = (ctypes.c_double * 3)(*SPACINGS[1])
    want_index, want_sq = transform._nearest_site_numpy(sites_np, SPACINGS[1])
    lib = N.lib

    need = lib.ru3d_edt_workspace_bytes(X, Y, Z)                             # the workspaces of include/ru3d.h
    need_without_sq, need_assign = need + 8 * voxels, 2 * lib.ru3d_skeleton_workspace_bytes(X, Y, Z)
    ws = torch.empty(max(need_without_sq, need_assign), dtype=torch.uint8, device=dev)
    bits = sites.bits.clone()
    _, index, index_ok = guarded(voxels, torch.int32, -77, dev)
    _, sq, sq_ok = guarded(voxels, torch.float64, -77.0, dev)
    assert lib.ru3d_nearest_site(bits.data_ptr(), X, Y, Z, spacing, index.data_ptr(), sq.data_ptr(), ws.data_ptr(), need,
                                 stream) == 0
    assert index_ok() and sq_ok() and torch.equal(bits, sites.bits)
    assert torch.equal(index.cpu(), torch.from_numpy(want_index.reshape(-1)))
    assert torch.equal(sq.cpu(), torch.from_numpy(want_sq.reshape(-1)))
    assert lib.ru3d_nearest_site(bits.data_ptr(), X, Y, Z, spacing, index.data_ptr(), sq.data_ptr(), ws.data_ptr(), need - 1,
                                 stream) < 0
    assert b"workspace" in lib.ru3d_last_error()
    # without sq the values live in the workspace: the small workspace is refused, the large one gives the same index
    assert lib.ru3d_nearest_site(bits.data_ptr(), X, Y, Z, spacing, index.data_ptr(), None, ws.data_ptr(),
                                 need_without_sq - 1, stream) < 0
    _, index2, index2_ok = guarded(voxels, torch.int32, -77, dev)
    assert lib.ru3d_nearest_site(bits.data_ptr(), X, Y, Z, spacing, index2.data_ptr(), None, ws.data_ptr(), need_without_sq,
                                 stream) == 0
    assert index2_ok() and torch.equal(index2, index)

    ids = torch.arange(1, n + 1, dtype=torch.int32, device=dev)
    kept = [t.clone() for t in (bits, region.bits, index, ids)]
    _, labels, labels_ok = guarded(voxels, torch.int32, -77, dev)
    need = need_assign

    def assign(count, ws_bytes=need, idx=index):
        return lib.ru3d_site_assign(bits.data_ptr(), region.bits.data_ptr(), idx.data_ptr(), ids.data_ptr(), count, X, Y, Z,
                                    labels.data_ptr(), ws.data_ptr(), ws_bytes, stream)

    assert assign(n) == 0 and labels_ok()
    want_labels = transform._site_assign_numpy(sites_np, np.arange(1, n + 1, dtype=np.int32), want_index, volume)
    assert torch.equal(labels.cpu(), torch.from_numpy(want_labels.reshape(-1)))
    assert assign(n, need - 1) < 0 and b"workspace" in lib.ru3d_last_error()
    assert assign(n - 1) < 0 and b"number of set bits" in lib.ru3d_last_error()          # seen on the device only
    assert labels_ok() and bool((labels == 0).all())
    wrong = index.clone()
    free = int(np.flatnonzero(volume.reshape(-1) & ~sites_np.reshape(-1))[0])           # a region voxel that is no site
    wrong[free] = free
    assert assign(n, need, wrong) < 0 and b"not a set voxel" in lib.ru3d_last_error() and labels_ok()
    assert all(torch.equal(a, b) for a, b in zip(kept, (bits, region.bits, index, ids)))

    assert assign(n) == 0
    other = on(dev, (np.indices(volume.shape).sum(axis=0) % 4).astype(np.uint8).reshape(-1))
    kept = [t.clone() for t in (labels, other, region.bits)]
    for K in (n, 30000):                                                    # the LDS table and the atomics beyond it
        cells = (K + 1) * 3
        _, table, table_ok = guarded(cells, torch.int64, -77, dev)
        tally_need = 256
        args = (labels.data_ptr(), K, other.data_ptr(), 2, region.bits.data_ptr(), X, Y, Z, table.data_ptr(), ws.data_ptr())
        assert lib.ru3d_territory_tally(*args, tally_need, stream) == 0 and table_ok()
        want = transform._territory_tally_numpy(want_labels, K, other.cpu().numpy().reshape(volume.shape), 2, volume)
        assert torch.equal(table.cpu(), torch.from_numpy(want.reshape(-1)))
        assert lib.ru3d_territory_tally(*args, tally_need - 1, stream) < 0 and b"workspace" in lib.ru3d_last_error()
        assert all(torch.equal(a, b) for a, b in zip(kept, (labels, other, region.bits)))
    _, table, table_ok = guarded((n // 2 + 1) * 3, torch.int64, -77, dev)   # labels above K: refused, nothing outside
    assert lib.ru3d_territory_tally(labels.data_ptr(), n // 2, other.data_ptr(), 2, region.bits.data_ptr(), X, Y, Z,
                                    table.data_ptr(), ws.data_ptr(), tally_need, stream) < 0
    assert b"outside 0 .. K" in lib.ru3d_last_error() and table_ok()

    with pytest.raises(N.Ru3dError):
        territory.assign(sites, ids[:-1], index.reshape(sites.shape), region)
    with pytest.raises(N.Ru3dError):
        territory.tally(labels.reshape(sites.shape), 3)
    with pytest.raises(ValueError):
        territory.nearest(torch.from_numpy(volume).to(dev))
    with pytest.raises(ValueError):
        territory.tally(labels.reshape(sites.shape), 3, None, 2)


def test_nearest_feature_on_hip_operands(dev):
    volume = np.zeros((20, 18, 70), dtype=np.uint8)
    volume[blob(0)] = 2
    for sampling in (None, (0.75, 0.5, 3.0), 2.0):
        want = transform.nearest_feature(volume, sampling)
        got = transform.nearest_feature(torch.from_numpy(volume).to(dev), sampling)
        assert all(g.is_cuda and torch.equal(g.cpu(), torch.from_numpy(w)) for g, w in zip(got, want))
    want = transform.nearest_feature(volume[3] != 0, (0.5, 2.0))
    got = transform.nearest_feature(torch.from_numpy(volume[3] != 0).to(dev), (0.5, 2.0))
    assert all(torch.equal(g.cpu(), torch.from_numpy(w)) for g, w in zip(got, want))


def organ_case():
    """The dilated Y of the skeleton tests as the vessel (1) inside a dilated organ (2) with a cube tumour (3)."""
    vessel = tree_case()['label'] == 1
    volume = np.zeros(vessel.shape, dtype=np.uint8)
    volume[ndi.binary_dilation(vessel, iterations=4)] = 2
    volume[18:22, 18:22, 9:13] = 3
    volume[vessel] = 1
    return volume


def test_territory_drivers_on_hip_operands(dev, tmp_path):
    volume = organ_case()
    affine = np.diag([0.75, 0.5, 3.0, 1.0])
    affine[:3, 3] = (-20.0, 4.0, 100.0)
    for options in (dict(vessel=1, organ=2, other=3), dict(vessel=1, organ=2, other=3, min_branch_mm=6.0, root=1),
                    dict(vessel=1, organ=(2, 3)), dict(vessel=1, organ=1), dict(vessel=3, organ=2, other=1)):
        want = trainer.vessel_territories_case({'pred': volume, 'affine': affine}, return_labels=True, **options)
        got = trainer.vessel_territories_case({'pred': torch.from_numpy(volume).to(dev), 'affine': affine},
                                              return_labels=True, **options)
        labels, want_labels = got.pop('labels'), want.pop('labels')
        assert labels.is_cuda and labels.dtype == torch.int32 and torch.equal(labels.cpu(), torch.from_numpy(want_labels))
        assert same(got, want)
        region = np.isin(volume, np.atleast_1d(options['organ']).tolist() + ([options['other']] if 'other' in options else []))
        assert want['organ_voxels'] == int(region.sum()) == int((want_labels > 0).sum()) + want['unassigned_voxels']

    (tmp_path / 'pred').mkdir()
    nifti.save(volume, affine, tmp_path / 'pred' / 'case_0.nii.gz')
    host = trainer.extract_vessel_territories(tmp_path / 'pred' / 'case_0.nii.gz', tmp_path / 'host', vessel=1, organ=2, other=3)
    device = trainer.extract_vessel_territories(tmp_path / 'pred' / 'case_0.nii.gz', tmp_path / 'device', device=dev, vessel=1,
                                                organ=2, other=3)
    assert host['branches'] == 3 and host['unassigned_voxels'] == 0
    for key in ('file', 'labels_file'):
        assert host[key].name == device[key].name
    assert host['file'].read_bytes() == device['file'].read_bytes()
    assert (nifti.load(host['labels_file'])[0] == nifti.load(device['labels_file'])[0]).all()
    assert same(json_load(device['file']), {k: v for k, v in device.items() if k not in ('file', 'labels_file')})
