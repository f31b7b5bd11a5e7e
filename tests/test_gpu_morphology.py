"""Packed masks and binary morphology on the HIP path (csrc/morphology.hip) against numpy / scipy on the same volumes.
Every comparison is exact: pack / unpack bit for bit (the tail bits of the packed words included), erosion, dilation,
opening and closing voxel for voxel with scipy.ndimage for both border values, and transform.post_transform on the
device against the host route and the reference's own output (tests/golden/g10_post.npz).  `-m gpu` only."""
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
import morphology  # noqa: E402
import transform  # noqa: E402

DEV = torch.device("cuda:0")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits_of(mask3):
    """The packed words (uint64 numpy [X, Y, W]) of a boolean [X, Y, Z] volume, built on the host."""
    X, Y, Z = mask3.shape
    W = (Z + 63) // 64
    padded = np.zeros((X, Y, W * 64), np.uint8)
    padded[:, :, :Z] = mask3
    return np.packbits(padded.reshape(X, Y, W, 64), axis=-1, bitorder="little").view("<u8").reshape(X, Y, W)


def _words(packed):
    return packed.bits.cpu().numpy().view(np.uint64)


def _ball(n):
    c = n // 2
    return transform.create_sphere((n, n, n), (c, c, c), c + (1 if n == 7 else 0)).astype(bool)


def _lop():
    s = np.zeros((3, 3, 3), bool)
    s[1, 1, 1] = s[2, 1, 1] = s[1, 1, 0] = True                  # centre, +x, -z: pins the reflection of a dilation
    return s


STRUCTURES = {"cross": None, "cube3": np.ones((3, 3, 3), bool), "ball7": _ball(7), "ball15": _ball(15),
              "bar_z": np.ones((1, 1, 15), bool), "bar_x": np.ones((15, 1, 1), bool), "bar_y": np.ones((1, 15, 1), bool),
              "lop": _lop()}


def _blobs(shape, seed):
    rng = np.random.RandomState(seed)
    return ndi.gaussian_filter(rng.standard_normal(shape), 2.5) > 0.02


def _both(mask, structure, border_value, iterations=1):
    """erosion and dilation of a boolean numpy volume on the device against scipy."""
    sc = ndi.generate_binary_structure(mask.ndim, 1) if structure is None else structure
    t = _dev(mask)
    for name in ("binary_erosion", "binary_dilation"):
        want = getattr(ndi, name)(mask, sc, iterations=iterations, border_value=border_value)
        got = getattr(transform, name)(t, structure, iterations=iterations, border_value=border_value)
        assert got.dtype == torch.bool and got.is_cuda and tuple(got.shape) == mask.shape
        differing = int((got.cpu().numpy() != want).sum())
        assert differing == 0, "%s: %d voxels differ from scipy" % (name, differing)


# ------------------------------------------------------------------------------------------------ pack / unpack
@pytest.mark.parametrize("Z", [1, 63, 64, 65, 130, 300, 256])
def test_pack_predicates_tail_bits_and_both_unpack_modes(Z):
    rng = np.random.RandomState(Z)
    v = rng.randint(0, 5, size=(5, 7, Z)).astype(np.uint8)
    t = _dev(v)
    for op, value, want in (("ne", 0, v != 0), ("eq", 2, v == 2), ("gt", 1, v > 1), ("ge", 3, v >= 3), ("ge", 0, v >= 0),
                            ("gt", 255, v > 255), ("eq", 0, v == 0)):
        packed = morphology.pack(t, op, value)
        assert packed.bits.dtype == torch.int64 and tuple(packed.bits.shape) == (5, 7, (Z + 63) // 64)
        assert packed.shape == v.shape
        assert np.array_equal(_words(packed), _bits_of(want)), (op, value)           # the bits at z >= Z are 0
        written = morphology.unpack(packed, value=9)
        assert written.dtype == torch.uint8 and np.array_equal(written.cpu().numpy(), np.where(want, 9, 0))
        painted = morphology.unpack(packed, value=200, out=t.clone(), paint=True)
        assert np.array_equal(painted.cpu().numpy(), np.where(want, 200, v))
        flags = morphology.unpack(packed, out=torch.empty(v.shape, dtype=torch.bool, device=DEV))
        assert flags.dtype == torch.bool and np.array_equal(flags.cpu().numpy(), want)
    assert np.array_equal(t.cpu().numpy(), v)


def test_pack_of_views_bool_and_fewer_axes():
    rng = np.random.RandomState(1)
    flat = _dev(rng.randint(0, 3, size=4 * 6 * 48 + 5).astype(np.uint8))
    view = flat[5:].reshape(4, 6, 48)                             # rows of 48 bytes from an odd address: the byte path
    assert view.data_ptr() % 16 != 0
    want = view.cpu().numpy() == 1
    packed = morphology.pack(view, "eq", 1)
    assert np.array_equal(_words(packed), _bits_of(want))
    out = torch.zeros(4 * 6 * 48 + 5, dtype=torch.uint8, device=DEV)
    morphology.unpack(packed, 1, out=out[5:].reshape(4, 6, 48))
    assert np.array_equal(out.cpu().numpy()[5:].reshape(4, 6, 48), want) and not out[:5].any()
    b = _dev(rng.rand(3, 70) < 0.5)
    packed = morphology.pack(b)
    assert packed.shape == (3, 70) and packed.shape3 == (1, 3, 70)
    assert np.array_equal(_words(packed), _bits_of(b.cpu().numpy()[None]))
    line = _dev((rng.rand(200) < 0.5).astype(np.uint8))
    assert np.array_equal(morphology.unpack(morphology.pack(line)).cpu().numpy(), line.cpu().numpy())


# ------------------------------------------------------------------------------------------------ erosion / dilation
@pytest.mark.parametrize("border_value", [0, 1])
@pytest.mark.parametrize("name", sorted(STRUCTURES))
def test_every_structure_on_speckle_and_blobs(name, border_value):
    rng = np.random.RandomState(len(name) + border_value)
    _both(rng.rand(37, 50, 91) < 0.5, STRUCTURES[name], border_value)
    _both(_blobs((37, 50, 91), 5), STRUCTURES[name], border_value)


@pytest.mark.parametrize("border_value", [0, 1])
@pytest.mark.parametrize("shape", [(1, 1, 300), (5, 1, 1), (3, 4, 65), (130, 67, 300), (9, 40, 64), (8, 32, 128)])
def test_shapes_smaller_than_the_halo_and_off_the_tile(shape, border_value):
    rng = np.random.RandomState(sum(shape))
    mask = rng.rand(*shape) < 0.6
    for name in ("cross", "ball7", "lop", "bar_z") + (("ball15",) if np.prod(shape) < 10 ** 6 else ()):
        _both(mask, STRUCTURES[name], border_value)


@pytest.mark.parametrize("border_value", [0, 1])
@pytest.mark.parametrize("fill", ["d0.05", "d0.95", "zeros", "ones"])
def test_densities_and_constant_volumes(fill, border_value):
    shape = (20, 33, 70)
    if fill.startswith("d"):
        mask = np.random.RandomState(9).rand(*shape) < float(fill[1:])
    else:
        mask = np.full(shape, fill == "ones")
    for name in ("cross", "ball7", "ball15"):
        _both(mask, STRUCTURES[name], border_value)


@pytest.mark.parametrize("iterations", [1, 2, 3])
def test_iterations_ping_pong_and_leave_the_input_alone(iterations):
    mask = _blobs((37, 50, 91), 8) | (np.random.RandomState(2).rand(37, 50, 91) < 0.05)
    for border_value in (0, 1):
        _both(mask, None, border_value, iterations)
        _both(mask, STRUCTURES["cube3"], border_value, iterations)
    packed = morphology.pack(_dev(mask))
    before = _words(packed).copy()
    out = morphology.erode(packed, iterations=iterations)
    assert out is not packed and np.array_equal(_words(packed), before)
    assert np.array_equal(_words(out), _bits_of(ndi.binary_erosion(mask, iterations=iterations)))


def test_lower_dimensional_volumes_take_scipys_default_structure():
    rng = np.random.RandomState(12)
    _both(rng.rand(40, 150) < 0.6, None, 0)
    _both(rng.rand(40, 150) < 0.6, np.ones((3, 5), bool), 1)
    _both(rng.rand(500) < 0.7, None, 0)
    _both(rng.rand(500) < 0.7, np.array([1, 1, 0, 0, 0], bool), 0)
    assert transform.binary_dilation(_dev(rng.rand(6, 7, 8).astype(np.float32) - 0.5)).dtype == torch.bool     # any dtype: != 0


# ------------------------------------------------------------------------------------------------ opening / closing
@pytest.mark.parametrize("border_value", [0, 1])
@pytest.mark.parametrize("iterations", [1, 2])
def test_opening_and_closing_equal_scipy(iterations, border_value):
    mask = _blobs((37, 50, 91), 21) ^ (np.random.RandomState(4).rand(37, 50, 91) < 0.03)
    t = _dev(mask)
    for name in ("cross", "ball7", "lop"):
        s = STRUCTURES[name]
        sc = ndi.generate_binary_structure(3, 1) if s is None else s
        want = ndi.binary_opening(mask, sc, iterations=iterations, border_value=border_value)
        assert np.array_equal(transform.binary_opening(t, s, iterations, border_value).cpu().numpy(), want), name
        want = ndi.binary_closing(mask, sc, iterations=iterations, border_value=border_value)
        assert np.array_equal(transform.binary_closing(t, s, iterations, border_value).cpu().numpy(), want), name


def test_closing_of_an_all_ones_volume_keeps_scipys_border_rule():
    ones = np.ones((9, 9, 9), bool)
    got = transform.binary_closing(_dev(ones), np.ones((3, 3, 3))).cpu().numpy()
    assert got.sum() == 343 and np.array_equal(got, ndi.binary_closing(ones, np.ones((3, 3, 3))))
    assert transform.binary_closing(_dev(ones), np.ones((3, 3, 3)), border_value=1).all()


def test_full_size_closing_with_the_ball_twice_the_same_words():
    x, y, z = np.ogrid[:512, :512, :256]
    rng = np.random.RandomState(0)
    mask = ((x - 200) / 120.0) ** 2 + ((y - 260) / 150.0) ** 2 + ((z - 120) / 90.0) ** 2 < 1
    mask ^= rng.rand(512, 512, 256) < 0.02
    mask[:40, 100:140, :] = True                                  # reaches three faces
    t = _dev(mask)
    packed = morphology.pack(t)
    first = morphology.close(packed, STRUCTURES["ball7"])
    second = morphology.close(packed, STRUCTURES["ball7"])
    assert torch.equal(first.bits, second.bits)
    want = ndi.binary_closing(mask, STRUCTURES["ball7"])
    assert np.array_equal(morphology.unpack(first).cpu().numpy().astype(bool), want)


# ------------------------------------------------------------------------------------------------ post_transform
def test_post_transform_device_equals_host_and_the_reference(golden_dir):
    z = np.load(os.path.join(golden_dir, "g10_post.npz"))
    t = _dev(z["input"])
    out = transform.post_transform(t)
    assert out.dtype == torch.uint8 and out.is_cuda and tuple(out.shape) == z["input"].shape
    assert np.array_equal(t.cpu().numpy(), z["input"]), "post_transform modified its input"
    assert np.array_equal(out.cpu().numpy(), z["post"])
    for kw in (dict(threshold=3000), dict(threshold=100, label=3, structure=np.ones((3, 3, 3))), dict(label=1)):
        want = transform.post_transform(z["input"].copy(), **kw)
        assert np.array_equal(transform.post_transform(t, **kw).cpu().numpy(), want), kw
    case = transform.PostTransform(threshold=3000)({"pred": t})
    assert np.array_equal(case["pred"].cpu().numpy(), transform.post_transform(z["input"].copy(), threshold=3000))
    empty = torch.zeros((12, 10, 70), dtype=torch.uint8, device=DEV)
    assert not transform.post_transform(empty).any()
    with pytest.raises(ValueError, match="uint8"):
        transform.post_transform(t.to(torch.int32))


# ------------------------------------------------------------------------------------------------ C ABI
def test_c_abi_refuses_bad_arguments_and_launches_nothing():
    lib = N.lib
    rng = np.random.RandomState(6)
    mask = rng.rand(6, 7, 70) < 0.5
    src = morphology.pack(_dev(mask))
    dst = src.new()
    dst.bits.fill_(-1)
    sentinel = dst.bits.clone()
    st = ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rows = (N.MorphRow * 1)(N.MorphRow(0, 0, 1 << 7))
    far = (N.MorphRow * 1)(N.MorphRow(0, -8, 1 << 7))
    wide = (N.MorphRow * 1)(N.MorphRow(0, 0, 1 << 15))
    bad = [lib.ru3d_binary_morph(p(src.bits), p(dst.bits), 6, 7, 70, N.MORPH_ERODE, far, 1, 0, st),
           lib.ru3d_binary_morph(p(src.bits), p(dst.bits), 6, 7, 70, N.MORPH_ERODE, wide, 1, 0, st),
           lib.ru3d_binary_morph(p(src.bits), p(dst.bits), 6, 7, 70, N.MORPH_ERODE, rows, 0, 0, st),
           lib.ru3d_binary_morph(p(src.bits), p(dst.bits), 6, 0, 70, N.MORPH_ERODE, rows, 1, 0, st),
           lib.ru3d_binary_morph(p(src.bits), None, 6, 7, 70, N.MORPH_ERODE, rows, 1, 0, st),
           lib.ru3d_binary_morph(None, p(dst.bits), 6, 7, 70, N.MORPH_ERODE, rows, 1, 0, st),
           lib.ru3d_binary_morph(p(src.bits), p(dst.bits), 6, 7, 70, N.MORPH_ERODE, None, 1, 0, st),
           lib.ru3d_binary_morph(p(dst.bits), p(dst.bits), 6, 7, 70, N.MORPH_ERODE, rows, 1, 0, st),
           lib.ru3d_binary_morph(p(src.bits), p(dst.bits), 6, 7, 70, 5, rows, 1, 0, st),
           lib.ru3d_binary_morph(p(src.bits), p(dst.bits), 6, 7, 70, N.MORPH_ERODE, rows, 1, 3, st),
           lib.ru3d_mask_pack(None, 6, 7, 70, N.MASK_NE, 0, p(dst.bits), st),
           lib.ru3d_mask_pack(p(src.bits), 6, 7, 70, 9, 0, p(dst.bits), st),
           lib.ru3d_mask_unpack(p(src.bits), 6, 7, 70, 300, 0, p(dst.bits), st)]
    table = torch.full((34, 34), -1, dtype=torch.int64, device=DEV)
    a = torch.zeros(64, dtype=torch.uint8, device=DEV)
    bad += [lib.ru3d_confusion_counts(p(a), p(a), 64, 33, p(table), st),
            lib.ru3d_confusion_counts(p(a), None, 64, 3, p(table), st),
            lib.ru3d_confusion_counts(p(a), p(a), -1, 3, p(table), st)]
    assert all(rc < 0 for rc in bad), bad
    torch.cuda.synchronize()
    assert torch.equal(dst.bits, sentinel) and bool((table == -1).all())
    # the identity structure through the raw entry point copies the volume (and the call still works after the refusals)
    assert lib.ru3d_binary_morph(p(src.bits), p(dst.bits), 6, 7, 70, N.MORPH_DILATE, rows, 1, 0, st) == 0
    assert torch.equal(dst.bits, src.bits)
    assert lib.ru3d_mask_bytes(6, 7, 70) == src.bits.numel() * 8


# ------------------------------------------------------------------------------------------------ CU budget
def test_confusion_counts_with_a_capped_grid():
    """ru3d_confusion_counts caps its grid-stride grid at 8 blocks a CU of the budget.  1000003 voxels, both operands
    16-byte aligned: 62500 vector trips + 3 tail voxels = 245 blocks of 256 threads uncapped, under the 2048 of the whole
    chip; under a budget of 8 CUs the cap is 64 and every thread makes three or four trips.  The table is np.bincount's,
    exactly (tests/test_gpu_evaluate.py's comparison), for an unaligned view (one voxel a trip: 3907 blocks uncapped) too."""
    n, C = 1000003, 3
    rng = np.random.RandomState(8)
    pred = rng.randint(0, C + 3, size=n + 1).astype(np.uint8)                 # values above C in either operand
    label = rng.randint(0, C + 2, size=n + 1).astype(np.uint8)

    def want(p, g):
        return np.bincount(np.minimum(g.astype(np.int64), C) * (C + 1) + np.minimum(p.astype(np.int64), C),
                           minlength=(C + 1) ** 2).reshape(C + 1, C + 1)
    dp, dl = _dev(pred), _dev(label)
    full = morphology.confusion(dp[:n], dl[:n], C)
    try:
        assert N.lib.ru3d_set_cu_budget(8) == 0
        got = morphology.confusion(dp[:n], dl[:n], C)
        odd = morphology.confusion(dp[1:], dl[:n], C)                         # operands that never reach a boundary together
    finally:
        N.lib.ru3d_set_cu_budget(0)
    assert N.lib.ru3d_get_cu_budget() == torch.cuda.get_device_properties(DEV).multi_processor_count
    assert np.array_equal(got.cpu().numpy(), want(pred[:n], label[:n])) and torch.equal(got, full)
    assert np.array_equal(odd.cpu().numpy(), want(pred[1:], label[:n]))
