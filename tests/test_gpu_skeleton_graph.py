"""GPU checks of csrc/skeleton_graph.hip and what is built on it: skeleton.graph (ids, node and branch tables, lengths,
chords, radii) with == against the numpy twin that defines it - word boundaries, thin and solid masks, the hand-made wire
figures and their translates, the skeleton fixtures, a capped grid - its repeatability, its memory contract (input bits,
capacity, a guard region), skeleton.prune against its twin, and the trainer's vessel-graph drivers on HIP operands
against the host route."""
import numpy as np
import pytest
import scipy.ndimage as ndi
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no HIP device", allow_module_level=True)

import _native as N  # noqa: E402
import morphology  # noqa: E402
import nifti  # noqa: E402
import skeleton  # noqa: E402
import trainer  # noqa: E402
import transform  # noqa: E402
from utils import json_load  # noqa: E402
from test_host_skeleton import FIXTURES, blob, thinned, tree_case  # noqa: E402
from test_host_skeleton_graph import FIGURES, place, same, spur_on_a_spur, wire_y  # noqa: E402

SPACINGS = [(1.0, 1.0, 1.0), (0.75, 0.5, 3.0)]          # dyadic: the squared distances are exact whichever feature ties
TABLES = ('n', 'nodes', 'branches', 'node_table', 'branch_table', 'length', 'chord', 'tortuosity')
RADII = ('radius_min', 'radius_mean', 'radius_max')


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def packed(volume, dev):
    return morphology.pack(torch.from_numpy(np.array(volume)).to(dev))      # a copy: the shared fixtures are read-only


def volume_of(mask):
    return morphology.unpack(mask).cpu().numpy().astype(bool)


def assert_same_graph(got, want, keys):
    assert got['ids'].dtype == torch.int32 and got['ids'].is_cuda
    assert torch.equal(got['ids'].cpu(), torch.from_numpy(want['ids']))
    for k in keys:
        assert same(got[k], want[k]), k
    assert set(got) == set(want)


def check_graph(volume, dev, mask=None, spacing=None):
    """skeleton.graph of `volume` against the twin with ==; the input bits stay what they were."""
    skel = packed(volume, dev)
    before = skel.bits.clone()
    volume3 = volume.reshape((1,) * (3 - volume.ndim) + volume.shape)
    spacing3 = (1.0,) * 3 if spacing is None else (1.0,) * (3 - len(spacing)) + tuple(spacing)
    if mask is None:
        got = skeleton.graph(skel, sampling=spacing)
        want = transform._skeleton_graph_numpy(volume3, None, spacing3)
        keys = TABLES
    else:
        got = skeleton.graph(skel, packed(mask, dev), spacing)
        sq = trainer._radii_squared_numpy(volume3, mask.reshape(volume3.shape), spacing3)
        want = transform._skeleton_graph_numpy(volume3, sq, spacing3)
        keys = TABLES + RADII
    assert torch.equal(skel.bits, before)
    assert_same_graph(got, want, keys)
    return got


@pytest.mark.parametrize("Z", [1, 2, 63, 64, 65, 130])
def test_graph_across_word_boundaries(dev, Z):
    volume = ndi.binary_dilation(np.random.RandomState(Z).rand(7, 9, Z) < 0.04, iterations=2)
    assert volume.any()
    check_graph(volume, dev)                                                # a mask that is not thin
    thin = transform._skeleton_numpy(volume)[0]
    for spacing in SPACINGS:
        check_graph(thin, dev, volume, spacing)


@pytest.mark.parametrize("name", sorted(FIGURES))
def test_graph_of_the_wire_figures_and_their_translates(dev, name):
    box = place(name)[0].shape
    big = (9, 10, 70)
    far = tuple(s - b for s, b in zip(big, box))
    for shape, offset in ((None, (0, 0, 0)), (big, (2, 1, 60)), (big, far)):
        volume, _ = place(name, shape, offset)                              # against the near faces, across z = 63 | 64 ..
        g = check_graph(volume, dev)                                        # .. and against the far faces
        assert (g['n'], g['nodes'], g['branches']) == tuple(len(FIGURES[name][k]) for k in ('voxels', 'nodes', 'branches'))
    check_graph(place(name, big, (2, 1, 60))[0], dev, spacing=(0.75, 0.5, 3.0))


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_graph_of_the_skeleton_fixtures(dev, name):
    volume, skel, _ = thinned(name)
    for spacing in SPACINGS:
        check_graph(skel, dev, volume, spacing)
    check_graph(volume, dev)


def test_graph_of_the_tree_case_and_fewer_axes(dev):
    for volume in tree_case().values():
        mask = volume == 1
        g = check_graph(transform._skeleton_numpy(mask)[0], dev, mask, SPACINGS[1])
        assert g['branches'] >= 1
    plane = np.zeros((9, 12), dtype=bool)
    plane[4, 1:11] = plane[1:8, 6] = True
    check_graph(plane, dev, spacing=(0.5, 2.0))
    check_graph(np.array([0, 1, 1, 1, 0, 1], dtype=bool), dev)
    empty = check_graph(np.zeros((3, 4, 5), dtype=bool), dev)
    assert (empty['n'], empty['nodes'], empty['branches']) == (0, 0, 0) and empty['ids'].numel() == 0


def test_radii_of_a_mask_without_background(dev):
    mask = np.ones((5, 6, 67), dtype=bool)
    wire = np.zeros_like(mask)
    wire[2, 3, 2:66] = True
    wire[2, 0:3, 30] = True                                                 # a side arm: an end, a path voxel, a junction voxel
    for spacing in SPACINGS:
        g = check_graph(wire, dev, mask, spacing)
        assert g['branches'] == 3 and np.isinf(g['radius_max']).all() and np.isinf(g['radius_mean']).all()
    g = check_graph(transform._skeleton_numpy(mask)[0], dev, mask)
    assert np.isinf(g['radius_min']).all()


def test_graph_with_a_capped_grid(dev):
    """The word loops (union, finalize, measure) cap their grid at 8 blocks a CU of the budget.  (136, 128, 64) is 17408
    words = 68 blocks of 256 threads uncapped; under a budget of 8 CUs the cap is 64, so 1024 words - and the set voxels
    in them - are done on the loops' second trip.  The mask is passed unthinned: one node holds most of its voxels."""
    volume = blob(11, (136, 128, 64))
    want = transform._skeleton_graph_numpy(volume)
    free = skeleton.graph(packed(volume, dev))
    assert_same_graph(free, want, TABLES)
    try:
        assert N.lib.ru3d_set_cu_budget(8) == 0
        capped = skeleton.graph(packed(volume, dev))
    finally:
        N.lib.ru3d_set_cu_budget(0)
    assert N.lib.ru3d_get_cu_budget() == torch.cuda.get_device_properties(dev).multi_processor_count
    assert_same_graph(capped, want, TABLES)
    assert torch.equal(capped['ids'], free['ids'])


def test_graph_is_repeatable(dev):
    volume = blob(7, (17, 19, 67))
    skel, mask = packed(transform._skeleton_numpy(volume)[0], dev), packed(volume, dev)
    a, b = skeleton.graph(skel, mask, SPACINGS[1]), skeleton.graph(skel, mask, SPACINGS[1])
    assert torch.equal(a['ids'], b['ids']) and all(same(a[k], b[k]) for k in TABLES + RADII)
    a, b = skeleton.graph(mask), skeleton.graph(mask)
    assert torch.equal(a['ids'], b['ids']) and all(same(a[k], b[k]) for k in TABLES)


def test_graph_arguments(dev):
    volume = place('y', (3, 9, 9), (1, 1, 1))[0]
    with pytest.raises(ValueError):
        skeleton.graph(torch.from_numpy(volume).to(dev))
    with pytest.raises(ValueError):
        skeleton.graph(packed(volume, dev), packed(np.ones((3, 9, 10), dtype=bool), dev))
    with pytest.raises(ValueError):
        skeleton.graph(packed(volume, dev), sampling=(1.0, 1.0))
    with pytest.raises(ValueError):
        skeleton.prune(torch.from_numpy(volume).to(dev), 1.0)
    with pytest.raises(ValueError):
        skeleton.prune(packed(volume, dev), -1.0)
    with pytest.raises(ValueError):
        skeleton.prune(packed(volume, dev), 1.0, max_rounds=-1)


def test_capacity_and_the_guard_region(dev):
    volume = transform._skeleton_numpy(blob(7, (17, 19, 67)))[0]
    want = transform._skeleton_graph_numpy(volume)
    n = want['n']
    skel = packed(volume, dev)
    X, Y, Z = skel.shape3
    ws = torch.empty(3 * N.lib.ru3d_skeleton_workspace_bytes(X, Y, Z), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def label(capacity):
        buf = torch.full((n + 64,), -77, dtype=torch.int32, device=dev)
        counts = torch.full((3,), -1, dtype=torch.int64, device=dev)
        rc = N.lib.ru3d_skeleton_graph_label(skel.bits.data_ptr(), X, Y, Z, buf.data_ptr() if capacity else None, capacity,
                                             counts.data_ptr(), ws.data_ptr(), ws.numel(), stream)
        assert rc == 0
        return buf.cpu().numpy(), counts.tolist()

    buf, counts = label(n)                                                  # exactly enough
    assert counts == [n, want['nodes'], want['branches']]
    assert (buf[:n] == want['ids']).all() and (buf[n:] == -77).all()
    for capacity in (n - 1, n // 2, 1, 0):                                  # too small: the count is still the true one
        buf, counts = label(capacity)
        assert counts == [n, 0, 0] and (buf == -77).all()

    # skeleton.graph grows its buffer and labels once more
    saved = skeleton._ids_capacity.get(dev)
    try:
        skeleton._ids_capacity[dev] = 16
        got = skeleton.graph(skel)
        assert skeleton._ids_capacity[dev] >= n
    finally:
        if saved is None:
            skeleton._ids_capacity.pop(dev, None)
        else:
            skeleton._ids_capacity[dev] = saved
    assert_same_graph(got, want, TABLES)


def check_prune(volume, dev, min_length, spacing=None, max_rounds=None):
    skel = packed(volume, dev)
    before = skel.bits.clone()
    got, rounds = skeleton.prune(skel, min_length, spacing, max_rounds)
    want = transform._skeleton_prune_numpy(volume, min_length, (1.0,) * 3 if spacing is None else spacing, max_rounds)
    assert torch.equal(skel.bits, before)                                   # the input is left alone
    assert got.shape == volume.shape and (volume_of(got) == want[0]).all() and rounds == want[1]
    Z = volume.shape[-1]
    if Z & 63:
        assert int((got.bits[..., -1] >> (Z & 63)).ne(0).sum().item()) == 0
    assert torch.equal(morphology.pack(morphology.unpack(got)).bits, got.bits)
    return want


def test_prune_against_the_twin(dev):
    skeletons = [transform._skeleton_numpy(tree_case()['label'] == 1)[0], transform._skeleton_numpy(blob(7, (17, 19, 67)))[0]]
    for volume in skeletons:
        lengths = transform._skeleton_graph_numpy(volume, None, SPACINGS[1])['length']
        for threshold in (0.0, float(np.median(lengths)), float(lengths.max()) + 1.0):
            check_prune(volume, dev, threshold, SPACINGS[1])
    assert check_prune(skeletons[1], dev, 0.0)[1] == 1
    assert int(check_prune(skeletons[1], dev, 1e9)[0].sum()) < int(skeletons[1].sum())


def test_prune_rounds_on_the_wire_figures(dev):
    volume, _ = wire_y(2)
    arm = 3 * np.sqrt(2.0)
    assert check_prune(volume, dev, arm)[1] == 1
    assert check_prune(volume, dev, float(np.nextafter(arm, 10.0)))[1] == 2
    moved = np.zeros((4, 24, 100), dtype=bool)
    moved[1:, :, 38:78] = spur_on_a_spur()                                  # the arm and its twig lie across z = 63 | 64
    assert check_prune(moved, dev, 12.0)[1] == 3
    assert check_prune(moved, dev, 12.0, max_rounds=1)[1] == 1
    assert check_prune(moved, dev, 12.0, max_rounds=0)[1] == 0


def test_vessel_graph_drivers_on_hip_operands(dev, tmp_path):
    case = tree_case()
    case['pred'][2:5, 2:5, 2:9] = 2                                         # a second structure the label does not have
    affine = np.diag([0.75, 0.5, 3.0, 1.0])
    affine[:3, 3] = (-20.0, 4.0, 100.0)
    for key in ('label', 'pred'):
        for threshold in (0.0, 6.0):
            want = trainer.vessel_graph_case({key: case[key], 'affine': affine}, key=key, min_branch_mm=threshold)
            on_device = torch.from_numpy(case[key]).to(dev)
            got = trainer.vessel_graph_case({key: on_device, 'affine': affine}, key=key, min_branch_mm=threshold)
            assert len(want) == (1 if key == 'label' else 2) and same(got, want)
    want = trainer.vessel_graph_case({'pred': case['pred'], 'affine': affine}, labels=[(1, 2)])
    assert same(trainer.vessel_graph_case({'pred': torch.from_numpy(case['pred']).to(dev), 'affine': affine}, labels=[(1, 2)]), want)

    (tmp_path / 'pred').mkdir()
    nifti.save(case['pred'], affine, tmp_path / 'pred' / 'case_0.nii.gz')
    host = trainer.extract_vessel_graph(tmp_path / 'pred' / 'case_0.nii.gz', tmp_path / 'host', min_branch_mm=6.0)
    device = trainer.extract_vessel_graph(tmp_path / 'pred' / 'case_0.nii.gz', tmp_path / 'device', device=dev, min_branch_mm=6.0)
    assert len(host) == len(device) == 2
    for h, d in zip(host, device):
        assert h['file'].name == d['file'].name and h['file'].read_bytes() == d['file'].read_bytes()
        assert same(json_load(d['file']), {k: v for k, v in d.items() if k != 'file'})
