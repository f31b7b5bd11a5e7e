"""Hole filling, propagation, keep-largest and the label clean-up on the HIP path (csrc/propagate.hip,
csrc/components.hip) against scipy / numpy on the same volumes.  Every comparison is exact, the tail bits of the packed
words included.  `-m gpu` only."""
import ctypes

import numpy as np
import pytest
import scipy.ndimage as ndi
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no HIP device", allow_module_level=True)

import _native as N  # noqa: E402
import components  # noqa: E402
import morphology  # noqa: E402
import trainer  # noqa: E402
import transform  # noqa: E402

import postprocess_cases as P  # noqa: E402

DEV = torch.device("cuda:0")
STRUCTURES = {"cross": 1, "cube": 3}
SENTINEL = 0x5A5A5A5A5A5A5A5A


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _structure(name, ndim):
    return None if name == "cross" else np.ones((3,) * ndim, dtype=bool)


def _bits_of(mask):
    """The packed words (uint64 numpy [X, Y, W]) of a boolean volume of 1 to 3 axes, built on the host."""
    mask3 = mask.reshape((1,) * (3 - mask.ndim) + mask.shape)
    X, Y, Z = mask3.shape
    W = (Z + 63) // 64
    padded = np.zeros((X, Y, W * 64), np.uint8)
    padded[:, :, :Z] = mask3
    return np.packbits(padded.reshape(X, Y, W, 64), axis=-1, bitorder="little").view("<u8").reshape(X, Y, W)


def _words(packed):
    return packed.bits.cpu().numpy().view(np.uint64)


def _fill(mask, name, expect=None):
    """morphology.fill_holes of a boolean numpy volume against scipy: the packed words, tail bits included; the operand
    unchanged; a second run the same bytes.  Returns the rounds the flood took."""
    structure = _structure(name, mask.ndim)
    want = ndi.binary_fill_holes(mask, structure=structure)
    if expect is not None:
        assert int(want.sum() - mask.sum()) == expect
    packed = morphology.pack(_dev(mask.astype(np.uint8)))
    before = _words(packed).copy()
    got = morphology.fill_holes(packed, structure)
    rounds = morphology.last_rounds
    assert got.shape == mask.shape and got.bits is not packed.bits
    words = _words(got)
    differing = int((words != _bits_of(want)).sum())
    assert differing == 0, "%d packed words differ from scipy (%s)" % (differing, name)
    assert np.array_equal(_words(packed), before), "fill_holes modified its operand"
    assert np.array_equal(_words(morphology.fill_holes(packed, structure)), words), "two runs differ"
    return rounds


# ------------------------------------------------------------------------------------------------ hole filling
VOLUMES = {
    "smooth_noise": (P.smooth_noise, (298, 75)),
    "dense_noise": (P.dense_noise, (11258, 2)),
    "box": (P.hollow_box, (288, 288)),
    "box_face_open": (lambda: P.hollow_box((2, 4, 34)), (0, 0)),
    "box_edge_open": (lambda: P.hollow_box((2, 2, 34)), (288, 0)),          # tells the two connectivities apart
    "serpentine_closed": (lambda: P.serpentine(False), (741, 741)),
}


@pytest.mark.parametrize("name", sorted(STRUCTURES))
@pytest.mark.parametrize("volume", sorted(VOLUMES))
def test_fill_holes_is_scipy(volume, name):
    make, expect = VOLUMES[volume]
    _fill(make(), name, expect[0 if name == "cross" else 1])


@pytest.mark.parametrize("name", sorted(STRUCTURES))
def test_the_opened_serpentine_needs_more_than_one_batch_of_rounds(name):
    rounds = _fill(P.serpentine(True), name, 0)
    assert rounds > 8, rounds                                                # 8 + 16 + ..: a second read-back at least
    assert morphology.last_rounds == rounds


@pytest.mark.parametrize("name", sorted(STRUCTURES))
def test_fill_holes_edge_cases(name):
    assert _fill(P.ring2d(), name, 64) >= 8
    line = np.array([0, 1, 0, 0, 1, 0], dtype=bool)
    _fill(line, name, 2)
    got = transform.binary_fill_holes(_dev(line.astype(np.uint8)), _structure(name, 1))
    assert got.dtype == torch.bool and got.cpu().tolist() == [False, True, True, True, True, False]
    for shape in ((5, 6, 70), (1, 1, 1), (1, 1, 64), (3, 3, 65)):
        _fill(np.ones(shape, bool), name, 0)
        _fill(np.zeros(shape, bool), name, 0)
    tail = np.ones((3, 3, 65), bool)                                          # a hole in the last voxel column but one
    tail[1, 1, 63] = tail[1, 1, 64] = False
    _fill(tail, name, 0)
    tail[:, :, 64] = True
    tail[1, 1, 64] = True
    _fill(tail, name, 1)
    ring3 = P.ring2d()[None]                                                  # as [1, Y, Z]: the x faces flood everything
    _fill(ring3, name, 0)


@pytest.mark.parametrize("name", sorted(STRUCTURES))
def test_transform_fill_holes_device_route(name):
    mask = P.smooth_noise()
    structure = _structure(name, 3)
    volume = _dev(mask.astype(np.uint8) * 3)                                  # any non-zero value is foreground
    before = volume.clone()
    got = transform.binary_fill_holes(volume, structure)
    assert got.dtype == torch.bool and got.is_cuda and tuple(got.shape) == mask.shape
    assert np.array_equal(got.cpu().numpy(), ndi.binary_fill_holes(mask, structure=structure))
    assert torch.equal(volume, before)
    as_bool = transform.binary_fill_holes(_dev(mask), structure)
    assert torch.equal(as_bool, got)


# ------------------------------------------------------------------------------------------------ propagation
@pytest.mark.parametrize("border_value", [0, 1])
@pytest.mark.parametrize("name", sorted(STRUCTURES))
def test_binary_propagation_is_scipy(name, border_value):
    allowed = P.smooth_noise()
    structure = _structure(name, 3)
    seed = np.zeros(allowed.shape, bool)
    inside = np.argwhere(allowed)
    outside = np.argwhere(~allowed & ndi.binary_dilation(allowed))           # not allowed, beside an allowed voxel
    seed[tuple(inside[len(inside) // 3])] = seed[tuple(inside[-1])] = seed[tuple(outside[len(outside) // 2])] = True
    want = ndi.binary_propagation(seed, structure=structure, mask=allowed, border_value=border_value)
    assert want.sum() > 3 and (border_value == 1 or want.sum() < allowed.sum())
    s, a = _dev(seed), _dev(allowed)
    got = transform.binary_propagation(s, structure, mask=a, border_value=border_value)
    assert got.dtype == torch.bool and np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(s.cpu().numpy(), seed) and np.array_equal(a.cpu().numpy(), allowed)
    ps, pa = morphology.pack(s), morphology.pack(a)
    words = (_words(ps).copy(), _words(pa).copy())
    reach = morphology.propagate(ps, pa, structure, border_value)
    assert np.array_equal(_words(reach), _bits_of(want))
    assert np.array_equal(_words(ps), words[0]) and np.array_equal(_words(pa), words[1])
    assert np.array_equal(_words(morphology.propagate(ps, pa, structure, border_value)), _words(reach))
    # no mask: everywhere; no seed: only the border floods
    everywhere = transform.binary_propagation(s, structure, border_value=border_value)
    assert bool(everywhere.all())
    flood = morphology.propagate(None, pa, structure, border_value)
    want = ndi.binary_propagation(np.zeros(allowed.shape, bool), structure=structure, mask=allowed, border_value=border_value)
    assert np.array_equal(_words(flood), _bits_of(want)) and bool(want.any()) == bool(border_value)


def test_propagation_on_a_mask_of_two_axes():
    allowed = ~P.ring2d()
    seed = np.zeros(allowed.shape, bool)
    seed[9, 64] = True                                                        # inside the ring
    for name in sorted(STRUCTURES):
        for border_value in (0, 1):
            structure = _structure(name, 2)
            want = ndi.binary_propagation(seed, structure=structure, mask=allowed, border_value=border_value)
            got = transform.binary_propagation(_dev(seed), structure, mask=_dev(allowed), border_value=border_value)
            assert np.array_equal(got.cpu().numpy(), want)
            assert int(want.sum()) == (64 if border_value == 0 else int(allowed.sum()))


# ------------------------------------------------------------------------------------------------ memory contract
def _guarded(words, fill=None):
    """int64 device buffer [guard | words | guard] with the guards set to the sentinel; returns (buffer, view, guard)."""
    guard = 64
    buf = torch.full((words + 2 * guard,), SENTINEL, dtype=torch.int64, device=DEV)
    view = buf[guard:guard + words]
    if fill is not None:
        view.copy_(fill.reshape(-1))
    return buf, view, guard


def _guards_intact(buf, guard):
    host = buf.cpu().numpy()
    return bool((host[:guard] == SENTINEL).all() and (host[-guard:] == SENTINEL).all())


@pytest.mark.parametrize("name", sorted(STRUCTURES))
def test_outputs_inside_a_larger_buffer_leave_the_sentinels_intact(name):
    mask = P.hollow_box((2, 2, 34))[:, :11, :]                                 # 12 x 11 x 70: rows and words end mid-tile
    structure = _structure(name, 3)
    want = ndi.binary_fill_holes(mask, structure=structure)
    packed = morphology.pack(_dev(mask.astype(np.uint8)))
    X, Y, Z = mask.shape
    n = packed.bits.numel()
    rbuf, reach, guard = _guarded(n, torch.zeros(n, dtype=torch.int64, device=DEV))
    obuf, out, _ = _guarded(n)
    cbuf = torch.full((8 + 2,), 77, dtype=torch.int32, device=DEV)
    stream = N.stream(DEV)
    for _ in range(3):
        N.check(N.lib.ru3d_binary_propagate(N.ptr(packed.bits), 1, ctypes.c_void_p(reach.data_ptr()), X, Y, Z,
                                            STRUCTURES[name], 7, 8, ctypes.c_void_p(cbuf.data_ptr() + 4), stream))
    N.check(N.lib.ru3d_mask_fill_result(N.ptr(packed.bits), ctypes.c_void_p(reach.data_ptr()),
                                        ctypes.c_void_p(out.data_ptr()), X, Y, Z, stream))
    torch.cuda.synchronize()
    assert _guards_intact(rbuf, guard) and _guards_intact(obuf, guard)
    counters = cbuf.cpu().numpy()
    assert counters[0] == 77 and counters[-1] == 77 and (counters[1:-1] == 0).all()      # converged, guards kept
    assert np.array_equal(out.cpu().numpy().view(np.uint64).reshape(X, Y, -1), _bits_of(want))
    assert np.array_equal(reach.cpu().numpy().view(np.uint64).reshape(X, Y, -1),
                          _bits_of(ndi.binary_propagation(np.zeros(mask.shape, bool), structure=structure, mask=~mask,
                                                          border_value=1)))


def test_fill_holes_allocates_packed_volumes_only():
    mask = np.ones((64, 64, 256), bool)
    mask[20:40, 20:40, 100:140] = False
    packed = morphology.pack(_dev(mask.astype(np.uint8)))
    volume = packed.bits.numel() * 8
    assert volume == 64 * 64 * 4 * 8
    morphology.fill_holes(packed)                                             # warm: the library and the allocator
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(DEV)
    start = torch.cuda.memory_allocated(DEV)
    got = morphology.fill_holes(packed)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated(DEV) - start
    assert grown <= 4 * volume + 64 * 1024, grown                             # a label volume would be 4 MB
    assert int(transform.binary_fill_holes(_dev(mask)).sum()) == mask.size and _words(got).all()


# ------------------------------------------------------------------------------------------------ keep the k largest
def _two_cubes():
    v = np.zeros((9, 10, 70), dtype=bool)
    v[1:4, 1:4, 2:5] = True                                                   # 27 voxels, numbered first
    v[5:8, 5:8, 62:65] = True                                                 # 27 voxels, across the word boundary
    v[1:3, 6:8, 30:33] = True                                                 # 12 voxels
    return v


KEEP_VOLUMES = {"dense_noise": P.dense_noise, "two_cubes": _two_cubes, "empty": lambda: np.zeros((5, 6, 70), bool)}


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("volume", sorted(KEEP_VOLUMES))
def test_keep_largest_against_the_numpy_twin(volume, k):
    mask = KEEP_VOLUMES[volume]()
    want_mask, want_labels = P.keep_largest_numpy(mask, k)
    m = _dev(mask.astype(np.uint8))
    labels, count = components.label(m)
    assert count == ndi.label(mask)[1]
    sizes, _ = components.stats(labels, count)
    labels_before = labels.clone()
    relabelled, kept = components.keep_largest(labels, count, sizes, k, mask=m, relabel=True)
    assert kept == min(k, count)
    assert np.array_equal(m.cpu().numpy().astype(bool), want_mask)
    assert np.array_equal(relabelled.cpu().numpy(), want_labels)              # a second ndi.label of the survivors
    assert torch.equal(labels, labels_before)
    if volume == "two_cubes" and k == 1:
        assert m[2, 2, 3] == 1 and m[6, 6, 63] == 0                           # equal sizes: the first-numbered cube
    # the public route, in place on a volume of any values
    values = _dev(mask.astype(np.uint8) * 5)
    out = transform.keep_largest_region(values, k)
    assert out is values and np.array_equal(values.cpu().numpy(), np.where(want_mask, 5, 0))
    as_float = _dev(mask.astype(np.float32) * 0.5)
    transform.keep_largest_region(as_float, k)
    assert np.array_equal(as_float.cpu().numpy() != 0, want_mask)


def test_keep_largest_keeps_everything_from_k_equal_count_on_and_honours_its_buffers():
    mask = _two_cubes()
    m = _dev(mask.astype(np.uint8))
    labels, count = components.label(m)
    assert count == 3
    sizes, _ = components.stats(labels, count)
    for k in (3, 4, 8):
        relabelled, kept = components.keep_largest(labels, count, sizes, k, mask=m, relabel=True)
        assert kept == 3 and torch.equal(relabelled, labels) and np.array_equal(m.cpu().numpy().astype(bool), mask)
    # raw call: mask, label output and workspace inside guarded buffers, the workspace exactly as large as asked for
    X, Y, Z = mask.shape
    n = mask.size
    need = N.lib.ru3d_filter_components_workspace_bytes(count)
    ws = torch.full((need + 512,), 0x5A, dtype=torch.uint8, device=DEV)
    mbuf = torch.full((n + 512,), 0x5A, dtype=torch.uint8, device=DEV)
    mbuf[256:256 + n] = m.reshape(-1)
    lbuf = torch.full((n + 128,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    kept = torch.full((3,), 99, dtype=torch.int32, device=DEV)
    N.check(N.lib.ru3d_keep_largest_components(N.ptr(labels), X, Y, Z, count, N.ptr(sizes), 2,
                                               ctypes.c_void_p(mbuf.data_ptr() + 256), ctypes.c_void_p(lbuf.data_ptr() + 256),
                                               ctypes.c_void_p(kept.data_ptr() + 4), ctypes.c_void_p(ws.data_ptr() + 256),
                                               need, N.stream(DEV)))
    torch.cuda.synchronize()
    want_mask, want_labels = P.keep_largest_numpy(mask, 2)
    assert kept.cpu().tolist() == [99, 2, 99]
    host = mbuf.cpu().numpy()
    assert (host[:256] == 0x5A).all() and (host[256 + n:] == 0x5A).all()
    assert np.array_equal(host[256:256 + n].reshape(mask.shape).astype(bool), want_mask)
    host = lbuf.cpu().numpy()
    assert (host[:64] == 0x5A5A5A5A).all() and (host[64 + n:] == 0x5A5A5A5A).all()
    assert np.array_equal(host[64:64 + n].reshape(mask.shape), want_labels)
    host = ws.cpu().numpy()
    assert (host[:256] == 0x5A).all() and (host[256 + need:] == 0x5A).all()


# ------------------------------------------------------------------------------------------------ clean_labels, the recipe
def test_clean_labels_device_route_equals_the_host_route():
    v = P.three_class_map()
    t = _dev(v)
    recipes = [
        {"fill_holes": (1, 3)},
        {"foreground": 2},
        {"foreground": 3, "keep_largest": {1: 2, 2: 1}, "min_voxels": {3: 10, 2: 2}, "fill_holes": [3, 1]},
        {"keep_largest": {1: 2}, "fill_holes": (1,), "structure": np.ones((3, 3, 3), bool)},
        {},
    ]
    changed = 0
    for recipe in recipes:
        want = transform.clean_labels(v, **recipe)
        got = transform.clean_labels(t, **recipe)
        assert got.dtype == torch.uint8 and got.is_cuda and got.data_ptr() != t.data_ptr()
        differing = int((got.cpu().numpy() != want).sum())
        assert differing == 0, "%r: %d voxels differ from the host route" % (recipe, differing)
        changed += int((want != v).sum() > 0)
    assert changed == 4 and np.array_equal(t.cpu().numpy(), v)
    filled = transform.clean_labels(t, fill_holes=(1,)).cpu().numpy()
    assert (filled[12:17, 9:14, 28:36] == 2).all() and (filled[14:18, 11:15, 44:50] == 1).all()
    case = transform.CleanLabels(foreground=2)({"pred": t})
    assert np.array_equal(case["pred"].cpu().numpy(), transform.clean_labels(v, foreground=2))
    kidney = _dev(P.toy_kidney())
    assert int((transform.clean_labels(kidney, fill_holes=(1,)) != kidney).sum()) == 12


def test_determine_postprocessing_on_the_device_returns_the_host_result(tmp_path):
    label_dir, pred_dir = P.write_validation_cases(tmp_path)
    for kwargs in ({}, {"data_range": [0]}, {"data_range": [1]}, {"fill_holes": (1,), "max_components": 3}):
        host = trainer.determine_postprocessing(label_dir, pred_dir, **kwargs)
        device = trainer.determine_postprocessing(label_dir, pred_dir, device=DEV, **kwargs)
        assert device == host, kwargs
    assert host["recipe"] == {"fill_holes": [1], "keep_largest": {1: 2}}
    written = trainer.batch_postprocess(pred_dir, str(tmp_path / "device"), host["recipe"], device=DEV)
    on_host = trainer.batch_postprocess(pred_dir, str(tmp_path / "host"), host["recipe"])
    import nifti
    for a, b in zip(written, on_host):
        assert np.array_equal(nifti.load(a)[0], nifti.load(b)[0])
