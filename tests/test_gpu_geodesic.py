"""GPU checks of csrc/geodesic.hip and what is built on it: geodesic.grow with == on both `dist` and `labels` against the
numpy twin that defines it (transform._geodesic_numpy) - word and tile boundaries, degenerate shapes, three spacings,
both connectivities, with and without a mask; corridors that cross tiles many times and one that winds inside a single
tile for longer than a round's trips; seeds outside the mask, adjacent and equidistant seeds, none, a negative one;
max_distance, the overflow flag and that a bound does not raise it; idle-tile skipping and repeatability byte for byte;
the memory contract (inputs, guard regions, short workspaces, bad arguments); transform.geodesic_distance and the
trainer's territory drivers with metric='geodesic' on HIP operands against the host route.

The wrapper's cases in the table of tests/test_gpu_scratch_contract.py (geodesic.grow, geodesic.grow_cube_limit) hold it to
that module's six checks.  Run with `-m gpu`."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no HIP device", allow_module_level=True)

import ctypes  # noqa: E402

import _native as N  # noqa: E402
import geodesic  # noqa: E402
import morphology  # noqa: E402
import trainer  # noqa: E402
import transform  # noqa: E402
from test_gpu_territory import SPACINGS, guarded, on, organ_case, packed  # noqa: E402
from test_host_geodesic import wall_case  # noqa: E402
from test_host_skeleton_graph import same  # noqa: E402

Q = 2.0 ** -10
NONE = 0xFFFFFFFF
CUBE = np.ones((3, 3, 3), dtype=bool)
TX, TY, TZ = N.GEODESIC_TILE


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def structure(connectivity, ndim=3):
    return None if connectivity == 1 else CUBE[(1,) * (3 - ndim)]


def twin(seeds, allowed, spacing, connectivity, quantum=Q, max_distance=None):
    shape3 = (1,) * (3 - seeds.ndim) + seeds.shape
    weights = geodesic.step_weights(spacing, seeds.ndim, connectivity, quantum)
    dist, labels = transform._geodesic_numpy(seeds.reshape(shape3), None if allowed is None else allowed.reshape(shape3), weights,
                                             geodesic.distance_limit(max_distance, quantum))
    return dist.reshape(seeds.shape), labels.reshape(seeds.shape)


def check_grow(dev, seeds, allowed, spacing=None, connectivity=1, want=None, **options):
    """geodesic.grow against the twin with == on dist and labels; the operands stay as they were."""
    s, a = on(dev, seeds), None if allowed is None else packed(allowed, dev)
    kept = [s.clone()] + ([a.bits.clone()] if a is not None else [])
    dist, labels = geodesic.grow(s, a, spacing, structure(connectivity, seeds.ndim), **options)
    assert dist.dtype == torch.uint32 and labels.dtype == torch.int32 and tuple(dist.shape) == tuple(labels.shape) == seeds.shape
    assert torch.equal(s, kept[0]) and (a is None or torch.equal(a.bits, kept[1]))
    if want is None:
        want = twin(seeds, allowed, spacing, connectivity, options.get('quantum', Q), options.get('max_distance'))
    got_dist, got_labels = dist.cpu().numpy(), labels.cpu().numpy()
    assert np.array_equal(got_dist, want[0]), "dist differs in %d voxels" % int((got_dist != want[0]).sum())
    assert np.array_equal(got_labels, want[1]), "labels differ in %d voxels" % int((got_labels != want[1]).sum())
    return got_dist, got_labels


def scattered(shape, seed, density, count=5):
    """(seeds int32 with `count` labelled voxels wherever they fall, allowed at `density`)"""
    rng = np.random.RandomState(seed)
    allowed = rng.rand(*shape) < density
    seeds = np.zeros(shape, dtype=np.int32)
    where = rng.choice(allowed.size, min(count, allowed.size), replace=False)
    seeds.reshape(-1)[where] = rng.randint(1, 9, len(where))
    return seeds, allowed


@pytest.mark.parametrize("Z", [1, 2, 63, 64, 65, 130])
def test_across_word_and_tile_boundaries(dev, Z):
    seeds, allowed = scattered((7, 9, Z), Z, 0.55)
    for i, spacing in enumerate(SPACINGS):
        for connectivity in (1, 3):
            check_grow(dev, seeds, allowed, spacing, connectivity)
        check_grow(dev, seeds, None, spacing, 1 + 2 * (i % 2))               # allowed=None: everywhere


@pytest.mark.parametrize("shape", [(1, 1, 300), (1, 300, 1), (300, 1, 1), (TX + 1, TY + 1, TZ + 1)])
def test_degenerate_shapes_and_one_voxel_more_than_a_tile(dev, shape):
    seeds = np.zeros(shape, dtype=np.int32)
    seeds.reshape(-1)[[3, seeds.size // 2 + 5]] = (4, 2)                    # two seeds: paths of more than a hundred steps
    allowed = np.ones(shape, dtype=bool)
    allowed.reshape(-1)[seeds.size - 7] = False                            # and a voxel that stops one of them
    for spacing in SPACINGS:
        for connectivity in (1, 3):
            dist, _ = check_grow(dev, seeds, allowed, spacing, connectivity)
        check_grow(dev, seeds, None, spacing, 3)
    assert (dist == NONE).sum() >= 1
    line = seeds.reshape(-1)                                                # fewer axes
    check_grow(dev, line, allowed.reshape(-1), 0.5, 1)
    if shape[0] == 1:
        check_grow(dev, seeds[0], allowed[0], (0.5, 2.0), 3)


def test_a_quarter_dense_mask_over_many_tiles(dev):
    seeds, allowed = scattered((33, 40, 70), 1, 0.25, count=9)
    reached = 0
    for spacing, connectivity in ((SPACINGS[1], 3), (SPACINGS[2], 3), (SPACINGS[0], 1)):
        dist, _ = check_grow(dev, seeds, allowed, spacing, connectivity)
        reached = max(reached, int((dist != NONE).sum()))
    assert reached > 10000                                                  # the cube's steps percolate at this density
    check_grow(dev, seeds, None, SPACINGS[1], 1)


def serpentine(shape):
    """(corridor, its voxels in path order): one voxel wide, rows along z at every other y of every other x, joined at
    alternating ends; by the face steps a voxel of it touches only the one before and the one after it on the path."""
    X, Y, Z = shape
    path, up_y, up_z = [], True, True
    for x in range(0, X, 2):
        ys = list(range(0, Y, 2)) if up_y else list(range(0, Y, 2))[::-1]
        for i, y in enumerate(ys):
            zs = list(range(Z)) if up_z else list(range(Z))[::-1]
            path += [(x, y, z) for z in zs]
            up_z = not up_z
            if i + 1 < len(ys):
                path.append((x, (y + ys[i + 1]) // 2, zs[-1]))
        up_y = not up_y
        if x + 2 < X:
            path.append((x + 1, ys[-1], path[-1][2]))
    corridor = np.zeros(shape, dtype=bool)
    corridor[tuple(np.array(path).T)] = True
    assert corridor.sum() == len(path)
    return corridor, path


@pytest.mark.parametrize("connectivity", [1, 3])
def test_a_corridor_that_crosses_tiles_many_times(dev, connectivity):
    corridor, path = serpentine((17, 17, 40))
    seeds = np.zeros(corridor.shape, dtype=np.int32)
    seeds[path[0]] = 3
    weights = geodesic.step_weights(SPACINGS[1], 3, connectivity, Q)
    dist, labels = check_grow(dev, seeds, corridor, SPACINGS[1], connectivity)
    assert geodesic.last_rounds > 1
    assert (labels[corridor] == 3).all() and (dist[~corridor] == NONE).all()
    # by hand, with the face steps: the corridor's own length, step by step
    if connectivity == 1:
        steps = np.abs(np.diff(np.array(path), axis=0))
        want = np.concatenate([[0], np.cumsum(steps @ np.array([weights[4], weights[10], weights[12]], dtype=np.int64))])
        assert (dist[tuple(np.array(path).T)] == want).all()
    # a row's 32 voxels inside a tile, entered at its end, take more trips than a round has
    assert N.GEODESIC_MAX_TRIPS <= TZ < corridor.shape[2]


def test_a_corridor_that_winds_inside_one_tile(dev):
    """540 steps inside the one tile of an (8, 8, 32) volume: every round stops at the cap of trips with the front
    somewhere in the tile, and the next round has to pick it up from the stored keys"""
    corridor, path = serpentine((TX, TY, TZ))
    seeds = np.zeros(corridor.shape, dtype=np.int32)
    seeds[path[-1]] = 7
    for connectivity in (1, 3):
        check_grow(dev, seeds, corridor, SPACINGS[2], connectivity)
        assert geodesic.last_rounds >= (len(path) - 1) // N.GEODESIC_MAX_TRIPS > 8
    check_grow(dev, seeds, corridor, SPACINGS[2], 1, skip_idle=False)


def test_seeds_outside_adjacent_equidistant_none_and_negative(dev):
    shape = (9, 12, 70)
    rng = np.random.RandomState(8)
    allowed = rng.rand(*shape) < 0.7
    allowed[4, 6, :] = True
    seeds = np.zeros(shape, dtype=np.int32)
    outside = np.argwhere(~allowed)[[5, 40, 77]]
    for label, p in zip((6, 2, 9), outside):                                # seeds outside `allowed` stay and spread
        seeds[tuple(p)] = label
    seeds[4, 6, 10], seeds[4, 6, 11] = 8, 3                                 # adjacent seeds with different labels
    seeds[4, 6, 30], seeds[4, 6, 38] = 5, 4                                 # (4, 6, 34) is as far from 5 as from 4
    for connectivity in (1, 3):
        dist, labels = check_grow(dev, seeds, allowed, SPACINGS[0], connectivity)
        assert labels[4, 6, 34] == 4 and dist[4, 6, 34] == 4 * 1024
        assert (labels[tuple(outside.T)] == (6, 2, 9)).all() and (dist[tuple(outside.T)] == 0).all()
        assert dist[4, 6, 10] == dist[4, 6, 11] == 0 and labels[4, 6, 9] == 8 and labels[4, 6, 12] == 3
    spread = [int((labels == l).sum()) for l in (6, 2, 9)]
    assert max(spread) > 1
    nothing = np.zeros(shape, dtype=np.int32)                               # no seed at all
    dist, labels = check_grow(dev, nothing, allowed, SPACINGS[1], 3)
    assert (dist == NONE).all() and (labels == 0).all()
    big = seeds.copy()
    big[0, 0, 0] = 0x7FFFFFFF                                               # the largest label
    check_grow(dev, big, None, SPACINGS[0], 1)
    seeds[2, 2, 2] = -1
    with pytest.raises(ValueError, match="negative"):
        geodesic.grow(on(dev, seeds), packed(allowed, dev))


def test_max_distance_and_the_overflow_flag(dev):
    seeds, allowed = scattered((9, 12, 70), 3, 0.8)
    for max_distance in (0.0, 3.0, 7.3, 1000.0):
        dist, _ = check_grow(dev, seeds, allowed, SPACINGS[2], 3, max_distance=max_distance)
        assert dist[dist != NONE].max() <= int(max_distance / Q)
    unbounded, _ = check_grow(dev, seeds, allowed, SPACINGS[2], 3)
    assert np.array_equal(dist, unbounded)                                  # a bound beyond every path changes nothing
    # steps of 2**20 quanta: the 4096th does not fit 32 bits
    line = np.zeros((1, 1, 5000), dtype=np.int32)
    line[0, 0, 0] = 1
    with pytest.raises(OverflowError, match="quantum"):
        geodesic.grow(on(dev, line), None, None, None, quantum=2.0 ** -20)
    # a bound stops the growth before that: no flag, and the twin's answer
    want = (np.where(np.arange(5000) <= 4000, np.arange(5000) << 20, NONE).astype(np.uint32).reshape(line.shape),
            (np.arange(5000) <= 4000).astype(np.int32).reshape(line.shape))
    check_grow(dev, line, None, None, 1, want=want, quantum=2.0 ** -20, max_distance=4000.0)
    dist, _ = check_grow(dev, line, None, None, 1, quantum=2.0 ** -19)       # and a coarser quantum fits
    assert dist[0, 0, 4999] == 4999 << 19
    with pytest.raises(ValueError, match="quantum"):
        geodesic.grow(on(dev, line), None, None, None, quantum=2.0 ** -21)


def test_idle_tile_skipping_and_repeatability(dev):
    seeds, allowed = scattered((33, 40, 70), 2, 0.3, count=4)
    corridor, path = serpentine((17, 17, 40))
    start = np.zeros(corridor.shape, dtype=np.int32)
    start[path[0]] = 1
    for s, a, connectivity in ((seeds, allowed, 3), (start, corridor, 1)):
        ds, da = on(dev, s), packed(a, dev)
        runs = [geodesic.grow(ds, da, SPACINGS[1], structure(connectivity), skip_idle=skip) for skip in (True, False, True)]
        for dist, labels in runs[1:]:
            assert torch.equal(dist.view(torch.int32), runs[0][0].view(torch.int32)) and torch.equal(labels, runs[0][1])
    check_grow(dev, seeds, allowed, SPACINGS[1], 3, skip_idle=False)


def test_memory_contract(dev):
    seeds_np, allowed_np = scattered((17, 19, 67), 7, 0.6)
    X, Y, Z = seeds_np.shape
    voxels = X * Y * Z
    stream = torch.cuda.current_stream(dev).cuda_stream
    lib = N.lib
    weights_np = geodesic.step_weights(SPACINGS[1], 3, 3, Q)
    weights = (ctypes.c_uint32 * 26)(*weights_np.tolist())
    want_dist, want_labels = transform._geodesic_numpy(seeds_np, allowed_np, weights_np, geodesic.UNLIMITED)
    seeds, allowed = on(dev, seeds_np.reshape(-1)), packed(allowed_np, dev)
    kept = [seeds.clone(), allowed.bits.clone()]
    need = lib.ru3d_geodesic_workspace_bytes(X, Y, Z)
    assert need == 2 * 256                                                  # 3 x 3 x 3 tiles, a byte each, rounded up
    _, keys, keys_ok = guarded(voxels, torch.int64, -77, dev)
    _, ws, ws_ok = guarded(need, torch.uint8, 0xA5, dev, pad=4096)
    _, dist, dist_ok = guarded(voxels, torch.int32, -77, dev)
    _, labels, labels_ok = guarded(voxels, torch.int32, -77, dev)
    _, changed, changed_ok = guarded(8, torch.int32, -77, dev)
    _, flags, flags_ok = guarded(2, torch.int32, -77, dev)
    guards = (keys_ok, ws_ok, dist_ok, labels_ok, changed_ok, flags_ok)

    def rounds(n=8, first=1, skip=1, ws_bytes=need, limit=geodesic.UNLIMITED, w=weights, allowed_ptr=allowed.bits.data_ptr()):
        return lib.ru3d_geodesic_rounds(allowed_ptr, 0, keys.data_ptr(), X, Y, Z, w, limit, n, first, skip, changed.data_ptr(),
                                        flags.data_ptr(), ws.data_ptr(), ws_bytes, stream)

    # refused with a status before anything is touched
    assert lib.ru3d_geodesic_init(seeds.data_ptr(), keys.data_ptr(), X, Y, Z, flags.data_ptr(), ws.data_ptr(), need - 1, stream) < 0
    assert b"workspace" in lib.ru3d_last_error()
    assert rounds(ws_bytes=need - 1) < 0 and b"workspace" in lib.ru3d_last_error()
    assert rounds(n=0) < 0 and rounds(n=65) < 0 and b"rounds" in lib.ru3d_last_error()
    assert rounds(limit=0xFFFFFFFF) < 0 and b"limit" in lib.ru3d_last_error()
    assert rounds(allowed_ptr=keys.data_ptr()) < 0 and b"one buffer" in lib.ru3d_last_error()
    heavy = (ctypes.c_uint32 * 26)(*weights_np.tolist())
    heavy[0] = (1 << 20) + 1
    assert rounds(w=heavy) < 0 and b"weight" in lib.ru3d_last_error()
    assert lib.ru3d_geodesic_split(keys.data_ptr(), dist.data_ptr(), dist.data_ptr(), X, Y, Z, stream) < 0
    torch.cuda.synchronize()
    assert all(ok() for ok in guards)
    assert bool((keys == -77).all()) and bool((ws == 0xA5).all()) and bool((changed == -77).all()) and bool((flags == -77).all())

    assert lib.ru3d_geodesic_init(seeds.data_ptr(), keys.data_ptr(), X, Y, Z, flags.data_ptr(), ws.data_ptr(), need, stream) == 0
    assert flags.tolist() == [0, 0] and bool((ws == 0).all())
    want_keys = np.where(seeds_np > 0, seeds_np.astype(np.int64), -1).reshape(-1)
    assert torch.equal(keys.cpu(), torch.from_numpy(want_keys))
    total, first = 0, 1
    while True:
        assert rounds(8, first, 1) == 0
        total, first = total + 8, 0
        counts = changed.tolist()
        assert all(c >= 0 for c in counts) and counts[0] <= 27
        if counts[-1] == 0:
            break
        assert total < 200
    assert rounds(3, 0, 1) == 0 and changed.tolist()[:3] == [0, 0, 0]       # an odd count of rounds on the fixpoint: only reads
    assert rounds(1, 0, 0) == 0 and changed.tolist()[0] == 0 and flags.tolist() == [0, 0]
    assert lib.ru3d_geodesic_split(keys.data_ptr(), dist.data_ptr(), labels.data_ptr(), X, Y, Z, stream) == 0
    torch.cuda.synchronize()
    assert all(ok() for ok in guards)
    assert np.array_equal(dist.cpu().numpy().view(np.uint32), want_dist.reshape(-1))
    assert np.array_equal(labels.cpu().numpy(), want_labels.reshape(-1))
    assert torch.equal(seeds, kept[0]) and torch.equal(allowed.bits, kept[1])

    with pytest.raises(ValueError):
        geodesic.grow(on(dev, seeds_np.astype(np.int64)), allowed)
    with pytest.raises(ValueError):
        geodesic.grow(on(dev, seeds_np), packed(allowed_np[:, :, :60], dev))
    with pytest.raises(ValueError):
        geodesic.grow(on(dev, seeds_np), on(dev, allowed_np))
    with pytest.raises(ValueError):
        geodesic.grow(on(dev, seeds_np), allowed, structure=np.ones((3, 3)))


def test_geodesic_distance_on_hip_operands(dev):
    seeds, allowed = scattered((20, 18, 70), 4, 0.5)
    for options in (dict(), dict(sampling=(0.75, 0.5, 3.0), structure=CUBE), dict(sampling=2.0, max_distance=31.0),
                    dict(sampling=(0.7, 0.9, 1.3), quantum=2.0 ** -6)):
        want = transform.geodesic_distance(seeds, allowed, **options)
        got = transform.geodesic_distance(on(dev, seeds), on(dev, allowed), **options)
        assert got[0].dtype == torch.float64 and got[1].dtype == torch.int32
        assert all(g.is_cuda and torch.equal(g.cpu(), torch.from_numpy(w)) for g, w in zip(got, want))
    want = transform.geodesic_distance(seeds[3].astype(np.uint8), None, (0.5, 2.0))
    got = transform.geodesic_distance(on(dev, seeds[3].astype(np.uint8)), None, (0.5, 2.0))
    assert all(torch.equal(g.cpu(), torch.from_numpy(w)) for g, w in zip(got, want))
    assert torch.isinf(transform.geodesic_distance(on(dev, np.zeros((5, 6), np.int32)))[0]).all()


def test_territory_drivers_with_the_geodesic_metric_on_hip_operands(dev, tmp_path):
    import nifti
    from utils import json_load
    affine = np.diag([0.75, 0.5, 3.0, 1.0])
    cases = [(organ_case(), dict(vessel=1, organ=2, other=3)), (organ_case(), dict(vessel=1, organ=2, min_branch_mm=6.0, root=1)),
             (organ_case(), dict(vessel=1, organ=1)), (wall_case(), dict(vessel=1, organ=2))]
    for volume, options in cases:
        want = trainer.vessel_territories_case({'pred': volume, 'affine': affine}, return_labels=True, metric='geodesic', **options)
        got = trainer.vessel_territories_case({'pred': torch.from_numpy(volume).to(dev), 'affine': affine}, return_labels=True,
                                              metric='geodesic', **options)
        labels, want_labels = got.pop('labels'), want.pop('labels')
        assert labels.is_cuda and labels.dtype == torch.int32 and torch.equal(labels.cpu(), torch.from_numpy(want_labels))
        assert same(got, want)
        assert want['organ_voxels'] == int((want_labels > 0).sum()) + want['unassigned_voxels']
    # the wall: the straight-line partition hands voxels to the vessel behind it, the geodesic one none - on the device
    volume = wall_case()
    both = [trainer.vessel_territories_case({'pred': torch.from_numpy(volume).to(dev), 'affine': np.eye(4)}, 1, 2,
                                            return_labels=True, metric=m)['labels'].cpu().numpy() for m in ('euclidean', 'geodesic')]
    a_half = (volume == 2) & (np.arange(24) < 14)[None, :, None]
    b_ids = np.unique(both[1][(volume == 2) & (np.arange(24) > 14)[None, :, None]])
    assert np.isin(both[0][a_half], b_ids).sum() > 300 and not np.isin(both[1][a_half], b_ids).any()

    (tmp_path / 'pred').mkdir()
    nifti.save(organ_case(), affine, tmp_path / 'pred' / 'case_0.nii.gz')
    host = trainer.extract_vessel_territories(tmp_path / 'pred' / 'case_0.nii.gz', tmp_path / 'host', vessel=1, organ=2, other=3,
                                              metric='geodesic')
    device = trainer.extract_vessel_territories(tmp_path / 'pred' / 'case_0.nii.gz', tmp_path / 'device', device=dev, vessel=1,
                                                organ=2, other=3, metric='geodesic')
    assert host['file'].read_bytes() == device['file'].read_bytes()
    assert (nifti.load(host['labels_file'])[0] == nifti.load(device['labels_file'])[0]).all()
    assert same(json_load(device['file']), {k: v for k, v in device.items() if k not in ('file', 'labels_file')})
