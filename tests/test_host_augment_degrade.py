"""CPU-only checks of the noise / blur / low-resolution ops of the patch sampler: the numpy twins (module `degrade`,
re-exported channels-last by `transform`) against known answers, scipy and `transform.resize`; the host draws of
DeviceAugment(noise=..., blur=..., low_res=...) under a scripted rng; the refusals of the constructor and of the C entry
point (no launch); header, binding and export of the three new symbols."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import scipy.ndimage as ndi
import torch

import _native as N
import augment
import degrade
import transform

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Script:
    """An rng that replays a list of (method, arguments, value) and fails on any call the list does not foresee."""

    def __init__(self, items):
        self.items = list(items)

    def _next(self, kind, args):
        assert self.items, "unexpected call %s%r" % (kind, args)
        want_kind, want_args, value = self.items.pop(0)
        assert (kind, args) == (want_kind, want_args), "expected %s%r, got %s%r" % (want_kind, want_args, kind, args)
        return value

    def uniform(self, *args):
        return self._next("uniform", args)

    def randint(self, *args):
        return self._next("randint", args)


class HostCase:
    """What DeviceAugment._draw reads of a case without a label: no kernel runs."""
    label = None

    def __init__(self, shape):
        self.shape = tuple(shape)
        self.image = torch.empty(0)


# ------------------------------------------------------------------------------------------------------- Philox
def test_philox_known_answers():
    cases = [((0, 0), (0, 0, 0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
             ((0xffffffff, 0xffffffff), (0xffffffff,) * 4, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
             ((0xa4093822, 0x299f31d0), (0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344),
              "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for key, counter, want in cases:
        got = transform.philox4x32(np.array(counter, dtype=np.uint64), key)
        assert got.dtype == np.uint32 and " ".join("%08x" % v for v in got) == want
    # vectorised over counters: the same words as one call each
    counters = np.array([c for _, c, _ in cases], dtype=np.uint64)
    many = degrade.philox4x32(counters, (0xa4093822, 0x299f31d0))
    assert " ".join("%08x" % v for v in many[2]) == cases[2][2]


def test_noise_statistics_and_keys():
    x = np.zeros((200000,), dtype=np.float32)[None, :, None, None]               # [C=1][x][1][1]
    a = degrade.gaussian_noise(x, 0.25, (7, 11))
    assert a.dtype == np.float32 and a.shape == x.shape
    n = a.ravel().astype(np.float64) / 0.5
    assert abs(n.mean()) <= 4.0 / np.sqrt(n.size)                                # 4 standard errors
    assert abs(n.var() - 1.0) <= 0.02
    assert np.array_equal(a, degrade.gaussian_noise(x, 0.25, (7, 11)))            # the same key: the same bits
    b = degrade.gaussian_noise(x, 0.25, (7, 12))
    assert (a != b).mean() > 0.99                                                 # another k1: another field
    assert (a != degrade.gaussian_noise(x, 0.25, (8, 11))).mean() > 0.99
    assert np.array_equal(degrade.gaussian_noise(x, 0.0, (7, 11)), x)


def test_noise_index_runs_over_channels_first():
    """transform.gaussian_noise takes [X, Y, Z, C]; voxel (c, x, y, z) takes normal number ((c X + x) Y + y) Z + z."""
    rng = np.random.RandomState(0)
    img = rng.randn(5, 4, 3, 2).astype(np.float32)
    got = transform.gaussian_noise(img, 0.04, (1, 2))
    normals = degrade.philox_normals(img.size, (1, 2)).reshape(2, 5, 4, 3)
    want = (np.moveaxis(img, -1, 0).astype(np.float64) + np.sqrt(0.04) * normals).astype(np.float32)
    assert got.shape == img.shape and np.array_equal(np.moveaxis(got, -1, 0), want)
    # one call yields four normals: the first call's, from the known answer for key 0, counter 0
    x = np.array([0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8], dtype=np.float64)
    ua, ub = (x[0] + 0.5) * 2.0 ** -32, (x[1] + 0.5) * 2.0 ** -32
    first = degrade.philox_normals(4, (0, 0))
    assert first[0] == np.sqrt(-2 * np.log(ua)) * np.cos(2 * np.pi * ub)
    assert first[1] == np.sqrt(-2 * np.log(ua)) * np.sin(2 * np.pi * ub)


# --------------------------------------------------------------------------------------------------------- blur
@pytest.mark.parametrize("shape", [(9, 7, 5), (19, 33, 70)])
@pytest.mark.parametrize("sigma", [0.5, 0.7, 1.0, 1.5])
def test_blur_against_scipy(shape, sigma):
    x = np.random.RandomState(1).randn(*shape).astype(np.float32)
    got = transform.gaussian_blur(x, sigma)
    want = ndi.gaussian_filter(x, sigma)
    assert got.dtype == np.float32 and got.shape == x.shape
    err = np.abs(got.astype(np.float64) - want.astype(np.float64)).max()
    print("blur %s sigma %g: max error %.3g, bound %.3g" % (shape, sigma, err, 3 * 2.0 ** -23 * np.abs(x).max()))
    assert err <= 3 * 2.0 ** -23 * np.abs(x).max()
    # channels-last: every channel on its own
    two = np.stack([x, -2 * x], axis=-1)
    both = transform.gaussian_blur(two, sigma)
    assert np.array_equal(both[..., 0], got) and np.array_equal(both[..., 1], transform.gaussian_blur(-2 * x, sigma))


def test_blur_radius_and_weights():
    assert [degrade.blur_radius(s) for s in (0.1, 0.5, 0.7, 1.0, 1.5, 4.0, 4.2)] == [0, 2, 3, 4, 6, 16, 17]
    w = degrade.blur_weights(1.5)
    assert len(w) == 7 and abs(w[0] + 2 * w[1:].sum() - 1.0) <= 1e-15
    x = np.random.RandomState(2).randn(6, 6, 6).astype(np.float32)
    assert np.array_equal(transform.gaussian_blur(x, 0.1), x)                     # radius 0: the identity


# ------------------------------------------------------------------------------------------------------ low-res
@pytest.mark.parametrize("shape,zoom", [((19, 33, 70), 0.5), ((19, 33, 70), 0.77), ((3, 4, 5), 0.5)])
def test_low_resolution_is_resize_down_and_up(shape, zoom):
    x = np.random.RandomState(3).randn(*shape).astype(np.float32)
    n = [max(int(np.round(p * zoom)), 2) for p in shape]
    assert degrade.low_grid(shape, zoom) == n
    want = transform.resize(transform.resize(x, n, order=0), list(shape), order=1)
    got = transform.simulate_low_resolution(x, zoom)
    assert got.dtype == np.float32 and want.shape == got.shape == x.shape
    assert np.array_equal(got, want)
    two = np.stack([x, 3 * x + 1], axis=-1)                                       # [X, Y, Z, C]
    both = transform.simulate_low_resolution(two, zoom)
    assert np.array_equal(both, transform.resize(transform.resize(two, n, order=0), list(shape), order=1))


def test_low_resolution_edge_cases():
    assert degrade.low_grid((3, 4, 5), 0.5) == [2, 2, 2]                          # 1.5 -> 2, 2.0, 2.5 -> 2 (half to even)
    s0, s1, w = degrade.low_res_taps(4, 2)                                        # low voxel 1 is source floor(3 + 0.5)
    assert s0.tolist() == [0, 0, 0, 3] and s1.tolist() == [3, 3, 3, 3] and np.allclose(w, [0, 1 / 3, 2 / 3, 0])
    s0, _, _ = degrade.low_res_taps(6, 3)                                         # low voxel 1: floor(2.5 + 0.5) = 3, the tie
    assert s0.tolist() == [0, 0, 0, 3, 3, 5]
    x = np.random.RandomState(4).randn(7, 9, 11).astype(np.float32)
    assert np.array_equal(transform.simulate_low_resolution(x, 1.0), x)           # zoom 1: the input bits
    for bad in (0.0, -0.5, 1.01):
        with pytest.raises(ValueError, match="zoom"):
            transform.simulate_low_resolution(x, bad)


# ---------------------------------------------------------------------------------------------------- draw order
SCALE = ("uniform", (1 - 0.1, 1 + 0.1), 1.0)
BOX = [("randint", (0, 24), 3), ("randint", (0, 20), 2), ("randint", (0, 16), 1)]
MIRROR = [("uniform", (), 0.7), ("uniform", (), 0.2), ("uniform", (), 0.9)]
INTENSITY = [("uniform", (0.9, 1.1), 1.05), ("uniform", (0.9, 1.1), 0.95), ("uniform", (0.9, 1.1), 1.0)]
KW = dict(scale=0.1, crop_size=16, crop_mode="random", contrast=[0.9, 1.1], brightness=[0.9, 1.1], gamma=[0.9, 1.1])
OPS = dict(noise=(0.1, (0.0, 0.1)), blur=(0.2, (0.5, 1.0)), low_res=(0.25, (0.5, 1.0)))


def test_draws_without_the_keywords_are_todays():
    script = Script([SCALE] + BOX + MIRROR + INTENSITY)
    drawn = augment.DeviceAugment(rng=script, **KW)._draw(HostCase((40, 36, 32, 1)))
    assert not script.items and len(drawn) == 3
    pr = drawn[0]
    assert list(pr.lo) == [3, 2, 1] and list(pr.flip) == [0, 1, 0] and pr.do_gamma == 1
    assert pr.contrast == np.float32(1.05) and pr.brightness == np.float32(0.95)


def test_new_draws_sit_between_mirror_and_contrast():
    new = [("uniform", (), 0.05), ("uniform", (0.0, 0.1), 0.04), ("randint", (0, 2 ** 31), 123), ("randint", (0, 2 ** 31), 456),
           ("uniform", (), 0.1), ("uniform", (0.5, 1.0), 0.8),
           ("uniform", (), 0.2), ("uniform", (0.5, 1.0), 0.6)]
    script = Script([SCALE] + BOX + MIRROR + new + INTENSITY)
    pr, _, geometry, dg = augment.DeviceAugment(rng=script, **KW, **OPS)._draw(HostCase((40, 36, 32, 1)))
    assert not script.items and geometry is None
    assert (dg.do_noise, dg.do_blur, dg.do_low_res) == (1, 1, 1) and list(dg.noise_key) == [123, 456]
    assert (dg.noise_variance, dg.blur_sigma, dg.low_res_zoom) == (0.04, 0.8, 0.6)
    assert pr.do_contrast == 1 and pr.contrast == np.float32(1.05)


def test_parameters_are_drawn_only_when_the_op_applies():
    # u == p does not apply (u < p); blur applies; low_res does not
    new = [("uniform", (), 0.1), ("uniform", (), 0.19), ("uniform", (0.5, 1.0), 0.75), ("uniform", (), 0.25)]
    script = Script([SCALE] + BOX + MIRROR + new + INTENSITY)
    dg = augment.DeviceAugment(rng=script, **KW, **OPS)._draw(HostCase((40, 36, 32, 1)))[3]
    assert not script.items and (dg.do_noise, dg.do_blur, dg.do_low_res) == (0, 1, 0) and dg.blur_sigma == 0.75
    # none applies: no parameters at all, the patch takes the one call it always took
    new = [("uniform", (), 0.5), ("uniform", (), 0.5), ("uniform", (), 0.5)]
    script = Script([SCALE] + BOX + MIRROR + new + INTENSITY)
    drawn = augment.DeviceAugment(rng=script, **KW, **OPS)._draw(HostCase((40, 36, 32, 1)))
    assert not script.items and len(drawn) == 4 and drawn[3] is None
    # only the configured ops draw
    new = [("uniform", (), 0.0), ("uniform", (0.5, 1.0), 1.0)]
    script = Script([SCALE] + BOX + MIRROR + new + INTENSITY)
    dg = augment.DeviceAugment(rng=script, **KW, low_res=OPS["low_res"])._draw(HostCase((40, 36, 32, 1)))[3]
    assert not script.items and (dg.do_noise, dg.do_blur, dg.do_low_res) == (0, 0, 1) and dg.low_res_zoom == 1.0


def test_transform_classes_make_the_same_draws():
    """RandomGaussianNoise / Blur / LowResolution on numpy's global generator: the stream DeviceAugment reads."""
    x = np.random.RandomState(5).randn(12, 10, 8, 2).astype(np.float32)
    chain = transform.Compose([transform.RandomGaussianNoise(1.0, (0.0, 0.1)), transform.RandomGaussianBlur(1.0, (0.5, 1.0)),
                               transform.RandomLowResolution(0.0, (0.5, 1.0))])
    np.random.seed(11)
    got = chain({"image": x.copy(), "label": None})["image"]
    after = np.random.uniform()
    np.random.seed(11)
    ops = degrade.draw(np.random, (1.0, (0.0, 0.1)), (1.0, (0.5, 1.0)), (0.0, (0.5, 1.0)))
    assert np.random.uniform() == after and sorted(ops) == ["blur", "noise"]
    want = transform.gaussian_blur(transform.gaussian_noise(x, *ops["noise"]), ops["blur"])
    assert np.array_equal(got, want) and not np.array_equal(got, x)


# ------------------------------------------------------------------------------------------------------ refusals
def test_constructor_refusals():
    augment.DeviceAugment(crop_size=64, blur=(0.2, (0.5, 4.0)))                   # radius 16
    augment.DeviceAugment(crop_size=[5, 33, 70], blur=(0.2, (0.5, 1.0)))          # radius 4 on an extent of 5
    with pytest.raises(ValueError, match="blur.*17.*16"):
        augment.DeviceAugment(crop_size=64, blur=(0.2, (0.5, 4.2)))
    with pytest.raises(ValueError, match="blur.*smallest patch extent 5"):
        augment.DeviceAugment(crop_size=[5, 33, 70], blur=(0.2, (0.5, 1.5)))
    for bad in ((0.25, (0.0, 1.0)), (0.25, (0.5, 1.5)), (0.25, (-0.5, 0.5)), (0.25, (0.9, 0.5))):
        with pytest.raises(ValueError, match="low_res"):
            augment.DeviceAugment(low_res=bad)
        with pytest.raises(ValueError, match="low_res"):
            transform.RandomLowResolution(*bad)
    for name, bad in (("noise", (0.1, (-0.1, 0.1))), ("noise", (1.5, (0.0, 0.1))), ("noise", 0.1), ("blur", (0.2, (0.0, 1.0))),
                      ("blur", (0.2, (0.5, float("nan")))), ("low_res", (0.25, 0.5))):
        with pytest.raises(ValueError, match=name):
            augment.DeviceAugment(**{name: bad})


def test_new_keywords_default_to_none_and_come_last():
    sig = inspect.signature(augment.DeviceAugment.__init__)
    assert list(sig.parameters)[-3:] == ["noise", "blur", "low_res"]
    assert all(sig.parameters[k].default is None for k in ("noise", "blur", "low_res"))
    plain = augment.DeviceAugment()
    assert plain.noise is None and plain.blur is None and plain.low_res is None and not plain.degrade


def test_header_library_and_binding_name_the_entry_points():
    text = open(os.path.join(ROOT, "include", "ru3d.h")).read()
    lib = ctypes.CDLL(N.LIB_PATH)
    for name, nargs in (("ru3d_augment_degrade_workspace_bytes", 4), ("ru3d_augment_degrade", 10), ("ru3d_augment_intensity", 6)):
        assert re.search(r"\b%s\s*\(" % name, text) and hasattr(lib, name)
        assert len(N.SIGNATURES[name][1]) == nargs
    assert "typedef struct ru3d_degrade_params" in text and "#define RU3D_DEGRADE_MAX_RADIUS 16" in text
    assert ctypes.sizeof(N.DegradeParams) == 6 * 4 + 3 * 8 and N.DegradeParams.noise_variance.offset == 24
    assert degrade.MAX_RADIUS == N.DEGRADE_MAX_RADIUS == 16
    assert "degrade.hip" in open(os.path.join(ROOT, "tools", "isa_check.py")).read()
    assert N.lib.ru3d_augment_degrade_workspace_bytes(2, 19, 33, 70) >= 2 * 19 * 33 * 70 * 4 + (19 + 33 + 70) * 16
    assert N.lib.ru3d_augment_degrade_workspace_bytes(0, 19, 33, 70) == 0


def test_c_argument_checks_answer_before_any_launch():
    lib = N.lib
    fake, other, third = ctypes.c_void_p(4096), ctypes.c_void_p(8192), ctypes.c_void_p(12288)   # never dereferenced
    big = 1 << 40

    def call(dg, image=fake, c=1, patch=(16, 16, 16), ws=other, ws_bytes=big, part=third):
        return lib.ru3d_augment_degrade(image, c, *patch, ctypes.byref(dg) if dg is not None else None, ws, ws_bytes, part,
                                        None)

    def failed(rc, word):
        return rc < 0 and word in lib.ru3d_last_error()

    def params(**kw):
        dg = N.DegradeParams()
        for k, v in kw.items():
            setattr(dg, k, v)
        return dg

    ok = params(do_blur=1, blur_sigma=1.0)
    assert failed(call(None), b"bad argument")
    assert failed(call(ok, image=None), b"bad argument")
    assert failed(call(ok, part=None), b"bad argument")
    assert failed(call(ok, c=0), b"bad argument")
    assert failed(call(ok, patch=(16, 0, 16)), b"empty patch")
    assert failed(call(ok, patch=(2048, 2048, 1024)), b"patch too large")
    assert failed(call(ok, ws_bytes=16 ** 3 * 4), b"workspace too small")
    assert failed(call(params(do_noise=1, noise_variance=-1.0)), b"noise_variance")
    assert failed(call(params(do_noise=1, noise_variance=float("nan"))), b"noise_variance")
    assert failed(call(params(do_blur=1, blur_sigma=0.0)), b"not positive")
    assert failed(call(params(do_blur=1, blur_sigma=4.2), patch=(64, 64, 64)), b"radius above 16")
    assert failed(call(params(do_blur=1, blur_sigma=float("inf")), patch=(64, 64, 64)), b"not positive")
    assert failed(call(params(do_blur=1, blur_sigma=1.5), patch=(5, 33, 70)), b"radius 6 exceeds the smallest patch extent 5")
    assert failed(call(params(do_low_res=1, low_res_zoom=0.0)), b"outside (0, 1]")
    assert failed(call(params(do_low_res=1, low_res_zoom=1.5)), b"outside (0, 1]")
    assert failed(call(params(do_low_res=1, low_res_zoom=float("nan"))), b"outside (0, 1]")
    assert failed(call(params(do_low_res=1, low_res_zoom=0.5), patch=(1, 16, 16)), b"at least 2 voxels")
    pr = N.PatchParams()
    assert failed(lib.ru3d_augment_intensity(None, 10, fake, 1, ctypes.byref(pr), None), b"bad argument")
    assert failed(lib.ru3d_augment_intensity(fake, 10, other, 0, ctypes.byref(pr), None), b"no partials")
    assert lib.ru3d_augment_intensity(fake, 10, other, 1, ctypes.byref(pr), None) == 0      # no flag set: nothing launched
