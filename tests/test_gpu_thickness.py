"""Local thickness on a real MI355X (csrc/thickness.hip), every comparison of T2 == against the numpy twin
transform._local_thickness_numpy, on the smallest shapes at which the kernels can go wrong: Z around the 64-bit word of
the packed mask and the 64 lanes of a row (1, 2, 63, 64, 65, 130), volumes of one row or one column, balls whose boxes
cross words and many rows (a neck between two balls; an ellipsoid whose half-extents differ sixfold between axes), the
empty, full, single-voxel and face-touching masks; repeatability, the work counters, the statistics and the drivers.

The memory contract of thickness.local_squared is held here with the six checks of tests/test_gpu_scratch_contract.py
(its docstring) at that file's VOL: that module's stand-ins and helpers are imported where they take the call as an
argument, and its four parametrised checks are restated for the one case.  The entry points are bound from
_native.SIGNATURES_SINCE, which that module's coverage tests do not see; the two coverage tests at the end of this
section stand in for them.
Run with `-m gpu`."""
import contextlib
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no HIP device", allow_module_level=True)

import _native as N  # noqa: E402
import distance  # noqa: E402
import morphology  # noqa: E402
import nifti  # noqa: E402
import skeleton  # noqa: E402
import thickness  # noqa: E402
import trainer  # noqa: E402
import transform  # noqa: E402
from utils import json_load  # noqa: E402
import test_gpu_scratch_contract as SC  # noqa: E402
from test_gpu_territory import SPACINGS, organ_case  # noqa: E402
from test_host_thickness import ball, opened, second_evaluation, two_balls  # noqa: E402

DEV = torch.device("cuda:0")
ULP2 = 2.0 ** -51


def pack(mask):
    return morphology.pack(torch.from_numpy(np.ascontiguousarray(mask).astype(np.uint8)).to(DEV))


def ellipsoid():
    """a solid ellipsoid in (20, 28, 70) for the spacing (0.75, 0.5, 3.0), half-axes 5, 5 and 81 in its units: the box of
    its largest ball reaches 7 voxels along x, 11 along y and 2 along z"""
    x, y, z = np.ogrid[:20, :28, :70]
    return ((x - 9.5) * 0.75 / 5.0) ** 2 + ((y - 13.5) * 0.5 / 5.0) ** 2 + ((z - 34.5) * 3.0 / 81.0) ** 2 < 1


@functools.lru_cache(maxsize=None)
def scene(name):
    mask = {"two_balls": two_balls, "ellipsoid": ellipsoid}[name]()
    assert 1000 < int(mask.sum()) <= 8000
    mask.setflags(write=False)
    return mask


@functools.lru_cache(maxsize=None)
def scene_twin(name, spacing):
    t2 = transform._local_thickness_numpy(scene(name), spacing)
    t2.setflags(write=False)
    return t2


def assert_t2(mask, spacing, what, sampling=None):
    """both painting orders against the twin of the mask as a volume of three axes"""
    shape3 = (1,) * (3 - mask.ndim) + mask.shape
    want = transform._local_thickness_numpy(mask.reshape(shape3), distance._spacing(spacing, mask.ndim)).reshape(mask.shape)
    p = pack(mask)
    for presort in (True, False):
        got = thickness.local_squared(p, spacing, presort=presort)
        assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == mask.shape, what
        assert np.array_equal(got.cpu().numpy(), want), "%s, presort=%s" % (what, presort)
    return want


# ------------------------------------------------------------------------------------------------ against the twin
@pytest.mark.parametrize("spacing", SPACINGS)
@pytest.mark.parametrize("Z", [1, 2, 63, 64, 65, 130])
def test_word_and_tile_boundaries(Z, spacing):
    mask = opened((7, 9, Z), seed=Z)
    assert mask.any() and not mask.all()
    want = assert_t2(mask, spacing, "(7, 9, %d) at %s" % (Z, spacing))
    assert (want[mask] > 0).all() and (want[~mask] == 0).all()


@pytest.mark.parametrize("shape", [(1, 1, 300), (1, 300, 1), (300, 1, 1), (300,), (300, 1), (1, 300)])
def test_degenerate_shapes_and_fewer_axes(shape):
    mask = opened(shape, seed=300, density=0.9)
    assert mask.any() and not mask.all()
    spacing = (0.7, 0.9, 1.3)[3 - len(shape):]
    want = assert_t2(mask, spacing, "%s" % (shape,))
    assert len(np.unique(want)) > 3                                     # runs of several lengths


@pytest.mark.parametrize("name,spacing", [("two_balls", (1.0, 1.0, 1.0)), ("two_balls", (0.7, 0.9, 1.3)),
                                          ("ellipsoid", (0.75, 0.5, 3.0))])
def test_balls_that_cross_words_and_many_rows(name, spacing):
    mask, want = scene(name), scene_twin(name, spacing)
    p = pack(mask)
    for presort in (True, False):
        got = thickness.local_squared(p, spacing, presort=presort).cpu().numpy()
        assert np.array_equal(got, want), (name, spacing, presort)
    if name == "two_balls" and spacing == (1.0, 1.0, 1.0):
        assert want[12, 12, 12] == 81 and want[12, 12, 36] == 36 and want[12, 12, 26] == 4
    r2 = thickness.inscribed_squared(p, spacing).cpu().numpy()
    assert np.array_equal(r2, transform._inscribed_squared_numpy(mask, spacing))
    assert (want[mask] >= r2[mask]).all() and set(want[mask].tolist()) <= set(r2[mask].tolist())


def test_special_masks():
    for shape in ((5, 6, 7), (3, 4, 64), (2, 3, 130)):
        empty = np.zeros(shape, dtype=bool)
        assert (assert_t2(empty, None, "empty %s" % (shape,)) == 0).all()
        full = np.ones(shape, dtype=bool)
        assert np.isposinf(assert_t2(full, (0.7, 0.9, 1.3), "full %s" % (shape,))).all()
        one = np.zeros(shape, dtype=bool)
        one[1, 2, shape[2] - 1] = True
        want = assert_t2(one, (0.75, 0.5, 3.0), "single voxel %s" % (shape,))
        assert want[1, 2, shape[2] - 1] == 0.25 and want.sum() == 0.25
        touching = np.ones(shape, dtype=bool)
        touching[1, 1, shape[2] // 2] = False
        want = assert_t2(touching, (0.7, 0.9, 1.3), "touching every face %s" % (shape,))
        assert np.isfinite(want).all() and (want[touching] > 0).all()


# ------------------------------------------------------------------------------------------------ work, repeatability
def test_repeatable_bytes_and_work_counters():
    mask, want = scene("two_balls"), scene_twin("two_balls", (1.0, 1.0, 1.0))
    pairs = second_evaluation(mask, (1.0, 1.0, 1.0))[2]
    p = pack(mask)
    runs = {}
    for presort in (True, False, True):
        got = thickness.local_squared(p, presort=presort, count_work=True)
        tested, issued = thickness.last_work
        print("two_balls presort=%s: %d voxels tested, %d atomics issued, %d covered pairs" % (presort, tested, issued, pairs))
        assert np.array_equal(got.cpu().numpy(), want)
        assert tested >= pairs and 0 < issued <= tested
        runs.setdefault(presort, []).append((got, tested))
    assert torch.equal(runs[True][0][0].view(torch.int64), runs[True][1][0].view(torch.int64))
    assert torch.equal(runs[True][0][0].view(torch.int64), runs[False][0][0].view(torch.int64))
    assert runs[True][0][1] == runs[True][1][1] == runs[False][0][1]        # the tests do not depend on the order
    thickness.local_squared(p)
    assert thickness.last_work is None
    # The order of the list shows where candidates follow one another: under the whole device the 3954 candidates of this
    # scene are all resident at once (one wavefront each), so the comparison runs under one CU's budget - 32 candidates
    # at a time - where the same bytes are due as well
    try:
        assert N.lib.ru3d_set_cu_budget(1) == 0
        atomics = {}
        for presort in (True, False):
            got = thickness.local_squared(p, presort=presort, count_work=True)
            assert np.array_equal(got.cpu().numpy(), want)
            atomics[presort] = thickness.last_work[1]
            assert thickness.last_work[0] == runs[True][0][1]
    finally:
        N.lib.ru3d_set_cu_budget(0)
    print("two_balls under one CU: %d atomics sorted, %d in element order" % (atomics[True], atomics[False]))
    assert atomics[True] <= atomics[False]


def test_candidates_and_paint_directly():
    """the two entry points on their own: the list in element order, a list in any order, a shortened list, capacity"""
    mask = scene("two_balls")
    p, want = pack(mask), scene_twin("two_balls", (1.0, 1.0, 1.0))
    index = thickness.candidates(p)
    assert index.dtype == torch.int32 and np.array_equal(index.cpu().numpy(), np.flatnonzero(mask))
    r2 = thickness.inscribed_squared(p)
    perm = torch.from_numpy(np.random.RandomState(0).permutation(index.numel())).to(DEV)
    got, _ = thickness.paint(r2, index[perm].contiguous(), mask.shape)
    assert np.array_equal(got.cpu().numpy(), want)
    # the centre of the large ball alone paints its ball
    centre = torch.tensor([(12 * 24 + 12) * 48 + 12], dtype=torch.int32, device=DEV)
    got, work = thickness.paint(r2, centre, mask.shape, count_work=True)
    assert np.array_equal(got.cpu().numpy(), np.where(ball(mask.shape, (12, 12, 12), 9), 81.0, 0.0))
    assert work.tolist()[1] == int(ball(mask.shape, (12, 12, 12), 9).sum())
    # capacity bounds the writes and the count says what was there
    X, Y, Z = mask.shape
    count = torch.empty(1, dtype=torch.int64, device=DEV)
    short = torch.full((100,), -7, dtype=torch.int32, device=DEV)
    ws = N.workspace(N.lib.ru3d_thickness_workspace_bytes(X, Y, Z), DEV)
    N.note_device(DEV)
    N.check(N.lib.ru3d_thickness_candidates(N.ptr(p.bits), X, Y, Z, N.ptr(short), 60, N.ptr(count), N.ptr(ws), ws.numel(),
                                            N.stream()), "thickness_candidates")
    assert int(count.item()) == int(mask.sum())
    assert np.array_equal(short[:60].cpu().numpy(), np.flatnonzero(mask)[:60]) and bool((short[60:] == -7).all())
    N.check(N.lib.ru3d_thickness_candidates(N.ptr(p.bits), X, Y, Z, None, 0, N.ptr(count), N.ptr(ws), ws.numel(), N.stream()),
            "thickness_candidates")
    assert int(count.item()) == int(mask.sum())


# ------------------------------------------------------------------------------------------------ memory contract
VOL = SC.VOL
CONTRACT_SPACING = (0.75, 0.5, 3.0)
QUERIES = ("ru3d_edt_workspace_bytes", "ru3d_thickness_workspace_bytes")
CALLED = set()


@functools.lru_cache(maxsize=None)
def contract_case():
    """(call, reference) in the form of SC's case table: thickness.local_squared on the solid of SC._volumes(), with the
    complement it takes R2 from among the outputs, so that its padding bits are looked at in every run"""
    host = SC._volumes()["solid"]
    assert tuple(host.shape) == VOL
    p = SC._pack(host)
    before = p.bits.clone()

    def call():
        t2 = thickness.local_squared(p, CONTRACT_SPACING, count_work=True)
        assert torch.equal(p.bits, before), "local_squared changed its operand"
        tested = thickness.last_work[0]               # the atomics issued may differ from run to run, the tests may not
        return dict(t2=t2, tested=[tested], complement=skeleton.complement(p),
                    unsorted=thickness.local_squared(p, CONTRACT_SPACING, presort=False))

    def reference(out):
        want = transform._local_thickness_numpy(host, CONTRACT_SPACING)
        assert np.array_equal(out["t2"].cpu().numpy(), want) and np.array_equal(out["unsorted"].cpu().numpy(), want)
        assert np.array_equal(SC._bools(out["complement"]), ~host)
    return call, reference


@contextlib.contextmanager
def recorded(into):
    """SC._recorded for the table it does not see: every entry point of _native.SIGNATURES_SINCE on N.lib, wrapped; the
    names called go `into`"""
    saved = {}
    for n in N.SIGNATURES_SINCE:
        saved[n] = fn = getattr(N.lib, n)

        def spy(*a, _fn=fn, _n=n):
            into.add(_n)
            return _fn(*a)
        setattr(N.lib, n, spy)
    try:
        yield
    finally:
        for n, fn in saved.items():
            setattr(N.lib, n, fn)


@functools.lru_cache(maxsize=None)
def clean():
    """checks 1 and 2: the clean run against the twin, then made again: the same launches, the same bits"""
    call, reference = contract_case()
    with recorded(CALLED):
        names, out, err = SC._run(call, "thickness.local_squared")
    assert err is None, err
    print("CLEAN thickness.local_squared %s" % names)
    reference(out)
    names2, out2, err2 = SC._run(call, "thickness.local_squared")
    assert err2 is None and names2 == names
    SC._same(out2, out, "thickness.local_squared: two consecutive clean runs (determinism)")
    return names, out


def test_contract_reference_then_determinism():
    names, out = clean()
    assert names == ["edt_squared", "thickness_candidates", "thickness_paint"] * 2
    SC._padding_clear(morphology.PackedMask(out["complement"], VOL), "complement")


def test_contract_leftovers_in_scratch_and_outputs():
    """check 3"""
    names, want = clean()
    call, _ = contract_case()
    for byte in SC.LEFTOVERS:
        what = "thickness.local_squared with 0x%02X left in the scratch and in what the wrapper allocates" % byte
        for buf in N._WS.values():
            buf.fill_(byte)
        got_names, out, err = SC._run(call, what, alloc=SC._Alloc(byte))
        assert err is None, err
        assert got_names == names
        SC._same(out, want, what)


def test_contract_scratch_of_exactly_the_asked_size():
    """check 4"""
    names, want = clean()
    call, _ = contract_case()
    scratch, alloc = SC._Scratch(), SC._Alloc(0xFF)
    with SC._spied(QUERIES) as seen:
        got_names, out, err = SC._run(call, "thickness.local_squared", scratch=scratch, alloc=alloc)
    print("SCRATCH thickness.local_squared: asked %s bytes; %s" % (scratch.queries, seen))
    assert err is None, err
    assert got_names == names
    SC._same(out, want, "thickness.local_squared on a scratch of exactly %s bytes" % scratch.queries)
    assert scratch.guard_intact(), "thickness.local_squared wrote behind the %s bytes it asked for" % scratch.queries
    for q, values in seen.items():
        assert values and all(v > 0 for v in values), "thickness.local_squared never asked %s" % q
    wanted = [v for values in seen.values() for v in values]
    assert not SC._matched(wanted, scratch.queries), (wanted, scratch.queries)
    assert seen["ru3d_thickness_workspace_bytes"] == [N.lib.ru3d_thickness_workspace_bytes(*VOL)] * 2


def test_contract_scratch_16_bytes_short_is_refused_before_any_launch():
    """check 5, for each ask of the call in turn"""
    clean_names, _ = clean()
    call, _ = contract_case()
    probe = SC._Scratch()
    SC._run(call, "thickness.local_squared", scratch=probe, alloc=SC._Alloc(0xFF))
    assert len(probe.queries) == 4 and min(probe.queries) >= SC.SHORT
    for k, asked in enumerate(probe.queries):
        alloc = SC._Alloc(0xFF)
        short = SC._Scratch(short=SC.SHORT, only=k, alloc=alloc)
        got_names, _, err = SC._run(call, "thickness.local_squared", scratch=short, alloc=alloc)
        what = "thickness.local_squared, ask %d (%d bytes) %d short" % (k, asked, SC.SHORT)
        print("SHORT %s: %s" % (what, err))
        assert err is not None, "%s: ran" % what
        assert got_names == [], "%s: launched %s after the ask and then refused" % (what, got_names)
        assert short.before == clean_names[:len(short.before)], "%s: launched %s ahead of the ask" % (what, short.before)
        if k == 0:
            assert short.before == [], "%s: launched %s ahead of its first ask" % (what, short.before)
        assert short.guard_intact(), "%s: wrote behind the scratch" % what
        assert alloc.unchanged_since(short.snap), "%s: wrote to what the wrapper had allocated" % what


def test_contract_misaligned_scratch_is_refused_before_any_launch():
    host = SC._volumes()["solid"]
    p = SC._pack(host)
    count = torch.full((1,), -1, dtype=torch.int64, device=DEV)
    ws = torch.empty(1024, dtype=torch.uint8, device=DEV)
    N.note_device(DEV)
    with SC.ops.launch_log() as log:
        rc = N.lib.ru3d_thickness_candidates(N.ptr(p.bits), *VOL, None, 0, N.ptr(count), ctypes.c_void_p(ws.data_ptr() + 4), 512,
                                             N.stream())
        torch.cuda.synchronize()
    assert rc != 0 and log.names == [] and int(count.item()) == -1
    assert b"aligned" in N.lib.ru3d_last_error()


def test_every_query_and_entry_point_of_the_new_table_is_held_here():
    """the two coverage tests of tests/test_gpu_scratch_contract.py, for _native.SIGNATURES_SINCE"""
    clean()
    wanted = {n for n in N.SIGNATURES_SINCE if n.endswith("_workspace_bytes") or n.endswith("_state_bytes")}
    assert wanted <= set(QUERIES), "no check for %s" % sorted(wanted - set(QUERIES))
    assert set(QUERIES) - wanted <= set(N.SIGNATURES)
    missing = sorted(set(N.SIGNATURES_SINCE) - CALLED)
    assert not missing, "not called by the clean run of the contract case: %s" % missing
    assert not set(N.SIGNATURES_SINCE) & set(N.SIGNATURES)


# ------------------------------------------------------------------------------------------------ statistics, front end
def test_summary_against_numpy():
    mask, t2 = scene("two_balls"), scene_twin("two_balls", (0.7, 0.9, 1.3))
    p, d_t2 = pack(mask), torch.from_numpy(np.array(t2)).to(DEV)
    got = thickness.summary(d_t2, p)
    want = trainer._thickness_stats_numpy(t2[mask])
    assert got['n'] == want['n'] == int(mask.sum()) <= 10 ** 5
    assert got['t2_min'] == want['t2_min'] and got['t2_max'] == want['t2_max'] and got['order'] == want['order']
    for key in ('mean', 'std'):
        print("summary %s: device %.17g, numpy %.17g" % (key, got[key], want[key]))
        assert abs(got[key] - want[key]) <= 1e-10 * abs(want[key])
    values = np.sort(t2[mask])
    for q, (lo, hi) in thickness.summary(d_t2, p, q=(0, 37.5, 100))['order'].items():
        ranks = trainer._percentile_ranks(values.size, q)
        assert (lo, hi) == (values[ranks[0]], values[ranks[1]])
    assert thickness.summary(torch.zeros(mask.shape, dtype=torch.float64, device=DEV), pack(np.zeros(mask.shape, bool))) == {'n': 0}
    assert trainer._thickness_metrics(got).keys() == trainer._thickness_metrics(want).keys()


def test_diameter_and_the_front_end_on_hip_tensors():
    mask = scene("ellipsoid")
    spacing = (0.75, 0.5, 3.0)
    t2 = scene_twin("ellipsoid", spacing)
    volume = torch.from_numpy(mask.astype(np.uint8) * 3).to(DEV)
    got_sq = transform.local_thickness(volume, spacing, squared=True)
    assert got_sq.is_cuda and got_sq.dtype == torch.float64 and np.array_equal(got_sq.cpu().numpy(), t2)
    want = transform.local_thickness(mask, spacing)
    assert np.array_equal(want, 2.0 * np.sqrt(t2))
    worst = 0.0
    for got in (transform.local_thickness(volume, spacing), thickness.diameter(got_sq)):
        got = got.cpu().numpy()
        assert np.array_equal(got == 0, want == 0)
        rel = np.abs(got - want)[mask] / want[mask]
        worst = max(worst, float(rel.max()))
        assert (rel <= ULP2).all()
    print("2 sqrt(T2): largest relative difference between the device and numpy %.3g (2^-52 = %.3g)" % (worst, 2.0 ** -52))
    line = torch.tensor([0, 1, 1, 1, 0, 0, 2, 2, 0], dtype=torch.uint8, device=DEV)
    assert transform.local_thickness(line, squared=True).tolist() == [0, 4, 4, 4, 0, 0, 1, 1, 0]
    assert transform.local_thickness(line, 0.5).tolist() == [0, 2, 2, 2, 0, 0, 1, 1, 0]
    assert math.isinf(float(transform.local_thickness(torch.ones(5, dtype=torch.uint8, device=DEV))[2]))


# ------------------------------------------------------------------------------------------------ drivers
def same_numbers(got, want):
    """the rules above on the dicts of thickness_case: counts and everything that comes from order statistics ==, mean
    and std (sums in another order) to 1e-10"""
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert set(g) - {'file'} == set(w) - {'file'} and g['label'] == w['label'] and g['voxels'] == w['voxels']
        for key in w:
            if key in ('mean', 'std'):
                assert abs(g[key] - w[key]) <= 1e-10 * abs(w[key]) + 1e-300, (key, g[key], w[key])
            elif key != 'file':
                assert g[key] == w[key], (key, g[key], w[key])


@functools.lru_cache(maxsize=None)
def organ():
    volume = organ_case()
    affine = np.diag([0.75, 0.5, 3.0, 1.0])
    affine[:3, 3] = (-20.0, 4.0, 100.0)
    host = trainer.thickness_case({'pred': volume, 'affine': affine}, return_map=True)
    return volume, affine, host


def test_thickness_case_on_hip_operands():
    volume, affine, (want, want_map) = organ()
    assert [r['label'] for r in want] == [1, 2, 3] and all(r['voxels'] for r in want)
    got, got_map = trainer.thickness_case({'pred': torch.from_numpy(volume).to(DEV), 'affine': affine}, return_map=True)
    same_numbers(got, want)
    assert isinstance(got_map, np.ndarray) and got_map.dtype == np.float32 and np.array_equal(got_map, want_map)
    assert (got_map[volume == 0] == 0).all() and (got_map[volume > 0] > 0).all()
    _, device_map = trainer.thickness_case({'pred': torch.from_numpy(volume).to(DEV), 'affine': affine}, labels=[(2, 3), 1],
                                           return_map=True, return_device=True)
    assert device_map.is_cuda and device_map.dtype == torch.float32 and tuple(device_map.shape) == volume.shape
    assert trainer.thickness_case({'pred': torch.from_numpy(volume).to(DEV), 'affine': affine}, labels=[9]) == [
        {'label': 9, 'voxels': 0}]


def test_measure_thickness_files(tmp_path):
    volume, affine, (want, want_map) = organ()
    (tmp_path / 'pred').mkdir()
    nifti.save(volume, affine, tmp_path / 'pred' / 'case_0.pred.nii.gz')
    device = trainer.measure_thickness(tmp_path / 'pred' / 'case_0.pred.nii.gz', tmp_path / 'device', device=DEV)
    same_numbers(device, want)
    assert [r['file'].name for r in device] == ['case_0.label_%d.thickness.json' % n for n in (1, 2, 3)]
    for r in device:
        same_numbers([dict(json_load(r['file']), label=r['label'])], [{k: v for k, v in r.items() if k != 'file'}])
    saved, saved_affine, _ = nifti.load(tmp_path / 'device' / 'case_0.thickness.nii.gz')
    assert np.array_equal(np.asarray(saved, dtype=np.float32), want_map) and np.allclose(saved_affine, affine)
    # the host route through the same drivers: the same numbers, and the same float32 map read back from its own file
    host = trainer.measure_thickness(tmp_path / 'pred' / 'case_0.pred.nii.gz', tmp_path / 'host')
    same_numbers(host, device)
    assert [r['file'].name for r in host] == [r['file'].name for r in device]
    host_saved, _, _ = nifti.load(tmp_path / 'host' / 'case_0.thickness.nii.gz')
    assert np.array_equal(np.asarray(host_saved, dtype=np.float32), np.asarray(saved, dtype=np.float32))
    # the batch driver, one structure, without a map
    batch = trainer.batch_measure_thickness(tmp_path / 'pred', tmp_path / 'batch', labels=[1], save_map=False)
    assert len(batch) == 1 and not (tmp_path / 'batch' / 'case_0.pred.thickness.nii.gz').exists()
    assert not list((tmp_path / 'batch').glob('*.nii.gz'))
    same_numbers(batch[0], device[:1])
    assert (tmp_path / 'batch' / 'case_0.label_1.thickness.json').exists()
