"""Host side of the blended sliding-window inference (inference.py: placement='cover', weighting='gaussian',
mirror_axes, model lists): the placement / weighting / ordering rules, the option checks, and fixture G12
(tests/golden/g12_tta.npz) pinned to the CPU oracle in float64.  No GPU."""
import inspect
import itertools
import math
import os

import numpy as np
import pytest
import torch

import inference as I
import network
import trainer as T
import _native as N
from oracle import unet_oracle as O


# --------------------------------------------------------------------------------------------------- placement
def test_cover_origins_rule_over_a_sweep():
    for P in (2, 3, 8, 16, 17, 96, 128):
        for s in (1, 2, 3, 4, 7):
            for L in sorted({P, P + 1, P + 2, P + P // s, P + P // s + 1, 2 * P - 1, 2 * P, 2 * P + 1, 3 * P + 5, 5 * P + 3}):
                o = I.cover_origins(L, P, s)
                n = math.ceil((L - P) * s / P) + 1
                assert len(o) == n == -((-(L - P) * s) // P) + 1, (L, P, s)
                assert o[0] == 0 and o[-1] == L - P
                steps = np.diff(o)
                assert (steps >= 0).all() and (len(steps) == 0 or steps.max() <= math.ceil(P / s)), (L, P, s, o)
                seen = np.zeros(L, dtype=bool)
                for v in o:
                    seen[v:v + P] = True
                assert seen.all(), (L, P, s, o)
                assert all(isinstance(v, int) for v in o)
    assert I.cover_origins(16, 16, 4) == [0]
    with pytest.raises(ValueError):
        I.cover_origins(15, 16, 2)
    with pytest.raises(ValueError):
        I.cover_origins(16, 16, 0)


def test_cover_origins_of_the_fixture_cases(golden_dir):
    want = {"a": [[0, 5], [0, 3], [0, 2, 5]], "b": [[0], [0, 8], [0, 2]], "d": [[0, 4], [0, 1], [0, 1]]}
    g6 = np.load(os.path.join(golden_dir, "g6_predict.npz"))
    g12 = np.load(os.path.join(golden_dir, "g12_tta.npz"))
    for tag, axes in want.items():
        patch = tuple(int(v) for v in g6[tag + "/patch"])
        full = I.padded_shape(g6[tag + "/image"].shape[:3], patch)
        assert [I.cover_origins(full[i], patch[i], 2) for i in range(3)] == axes
        origins, counts = I.cover_window_origins(full, patch, 2)
        assert counts == [len(a) for a in axes]
        assert origins == [tuple(v) for v in itertools.product(*axes)]          # x outer, z inner
        assert np.array_equal(g12[tag + "/origins"], np.array(origins))


# --------------------------------------------------------------------------------------------------- weighting
def test_gaussian_profile():
    for P in (8, 16, 17, 96, 128):
        for sc in (0.125, 0.25, 1.0):
            g = I.gaussian_profile(P, sc)
            assert g.dtype == np.float32 and g.shape == (P,)
            i = np.arange(P, dtype=np.float64)
            want = np.exp(-0.5 * ((i - (P - 1) / 2) / (sc * P)) ** 2)
            assert np.array_equal(g, want.astype(np.float32))
            assert np.array_equal(g, g[::-1])
            assert g.argmax() in ((P - 1) // 2, P // 2) and g.max() == g[(P - 1) // 2] == g[P // 2]
            assert (np.diff(g[:P // 2 + 1]) >= 0).all()
    assert np.array_equal(I.gaussian_profile(16), I.gaussian_profile(16, 0.125))
    # the window corner is a normal fp32 number: nothing to clamp, nothing flushed
    tiny = np.finfo(np.float32).tiny
    for patch in ((16, 16, 8), (96, 96, 96), (128, 128, 128), (240, 240, 80)):
        gx, gy, gz = (I.gaussian_profile(p) for p in patch)
        corner = np.float32(np.float32(gx[0] * gy[0]) * gz[0])
        assert tiny < corner < 3e-9 and corner >= np.float32(math.exp(-24.0)) * np.float32(0.99)
    with pytest.raises(ValueError):
        I.gaussian_profile(16, 0.0)


def test_mirror_subsets_order():
    assert I.mirror_subsets(()) == [()]
    assert I.mirror_subsets((1,)) == [(), (1,)]
    assert I.mirror_subsets((0, 2)) == [(), (0,), (2,), (0, 2)]
    assert I.mirror_subsets((2, 0)) == [(), (0,), (2,), (0, 2)]
    assert I.mirror_subsets((0, 1, 2)) == [(), (0,), (1,), (2,), (0, 1), (0, 2), (1, 2), (0, 1, 2)]


# --------------------------------------------------------------------------------------------------- fixture G12
def _merge_float64(image, weight_sets, pool, ncls, patch, weighting, mirror_axes, step=2):
    """The merge rule of the issue restated in numpy float64 on `oracle.unet_forward`; deliberately shares no code
    with inference.py beyond nothing at all."""
    orig = image.shape[:3]
    full = tuple(max(o, p) for o, p in zip(orig, patch))
    lo = tuple((f - o + 1) // 2 for o, f in zip(orig, full))                      # pad puts the odd voxel in front
    vol = np.zeros(full + (image.shape[3],))
    vol[lo[0]:lo[0] + orig[0], lo[1]:lo[1] + orig[1], lo[2]:lo[2] + orig[2]] = image
    axes = []
    for L, P in zip(full, patch):
        n = math.ceil((L - P) * step / P) + 1
        axes.append([0] if n == 1 else [(i * (L - P)) // (n - 1) for i in range(n)])
    w = np.ones(patch)
    if weighting == "gaussian":
        g = [np.exp(-0.5 * ((np.arange(P) - (P - 1) / 2) / (0.125 * P)) ** 2).astype(np.float32).astype(np.float64)
             for P in patch]
        w = g[0][:, None, None] * g[1][None, :, None] * g[2][None, None, :]
    subsets = [c for r in range(len(mirror_axes) + 1) for c in itertools.combinations(sorted(mirror_axes), r)]
    acc, cnt, terms = np.zeros(full + (ncls,)), np.zeros(full), np.zeros(full, dtype=np.int64)
    x = torch.from_numpy(np.moveaxis(vol, -1, 0)[None].copy())
    with torch.no_grad():
        for wts in weight_sets:
            for ox, oy, oz in itertools.product(*axes):
                sl = (slice(ox, ox + patch[0]), slice(oy, oy + patch[1]), slice(oz, oz + patch[2]))
                win = x[(slice(None), slice(None)) + sl]
                for sub in subsets:
                    dims = [2 + a for a in sub]
                    out = O.unet_forward(torch.flip(win, dims) if dims else win, wts, pool)
                    out = torch.sigmoid(out) if ncls == 1 else torch.softmax(out, dim=1)
                    out = torch.flip(out, dims) if dims else out
                    acc[sl] += np.moveaxis(out[0].numpy(), 0, -1) * w[..., None]
                    cnt[sl] += w
                    terms[sl] += 1
    crop = tuple(slice(lo[i], lo[i] + orig[i]) for i in range(3))
    return (acc / cnt[..., None])[crop], int(terms.max())


@pytest.mark.parametrize("tag,config,weighting,mirror_axes,sets,most_terms", [
    ("a", "cover_gaussian_m012", "gaussian", (0, 1, 2), 1, 96),
    ("d", "cover_gaussian_m02_ens", "gaussian", (0, 2), 2, 64),
    ("b", "cover_uniform", "uniform", (), 1, 4),
])
def test_g12_matches_the_oracle_in_float64(golden_dir, tag, config, weighting, mirror_axes, sets, most_terms):
    """The fixture is the float32 rounding of a float64 result of the reference's network; the oracle reproduces that
    float64 result to 1e-9, so it is within 1e-9 plus half a float32 ulp of what is stored."""
    g6 = np.load(os.path.join(golden_dir, "g6_predict.npz"))
    g12 = np.load(os.path.join(golden_dir, "g12_tta.npz"))
    patch = tuple(int(v) for v in g6[tag + "/patch"])
    _, pool, _, ncls = (int(v) for v in g6[tag + "/meta"])
    weight_sets = [{k[len(tag) + len(p):]: torch.from_numpy(z[k]).double() for k in z.files if k.startswith(tag + p)}
                   for z, p in ((g6, "/w/"), (g12, "/w2/"))][:sets]
    assert all(set(ws) == set(weight_sets[0]) and len(ws) > 0 for ws in weight_sets)
    prob, k = _merge_float64(g6[tag + "/image"].astype(np.float64), weight_sets, pool, ncls, patch, weighting, mirror_axes)
    assert k == most_terms
    fx, fm = g12["%s/%s/prob" % (tag, config)], g12["%s/%s/mask" % (tag, config)]
    assert fx.dtype == np.float32 and fx.shape == prob.shape == g6[tag + "/image"].shape[:3] + (ncls,)
    assert np.isfinite(fx).all()
    err = np.abs(prob - fx.astype(np.float64))
    print("g12 %s/%s: max |oracle - fixture| %.3g" % (tag, config, err.max()))
    assert (err <= 1e-9 + 0.5 * np.spacing(fx).astype(np.float64)).all()
    mask = np.round(prob[..., 0]) if ncls == 1 else prob.argmax(-1)
    assert fm.dtype == np.uint8 and np.array_equal(fm, mask.astype(np.uint8))


def test_g12_holds_every_configuration_and_all_classes(golden_dir):
    g12 = np.load(os.path.join(golden_dir, "g12_tta.npz"))
    for tag in ("a", "b", "d"):
        for config in ("cover_uniform", "cover_gaussian", "cover_gaussian_m012", "cover_gaussian_m02_ens"):
            p = g12["%s/%s/prob" % (tag, config)]
            assert np.isfinite(p).all() and p.min() >= 0 and p.max() <= 1
            if p.shape[-1] > 1:
                assert np.abs(p.sum(-1) - 1).max() < 1e-6
    assert np.unique(g12["a/cover_gaussian_m012/mask"]).tolist() == [0, 1, 2]
    assert g12["b/cover_uniform/prob"].shape[0] == 11                       # the odd pad: 11 -> 16 on axis 0


# --------------------------------------------------------------------------------------------------- options
def _cpu_model(ncls=2):
    return network.ResUnet3D(num_pool=1, num_features=4, in_channels=1, out_channels=ncls)


@pytest.mark.parametrize("kw,name", [
    (dict(placement="covering"), "placement"),
    (dict(weighting="hann"), "weighting"),
    (dict(mirror_axes=(0, 3)), "mirror_axes"),
    (dict(mirror_axes=(-1,)), "mirror_axes"),
    (dict(mirror_axes=(1, 1)), "mirror_axes"),
    (dict(mirror_axes=(0.5,)), "mirror_axes"),
    (dict(sigma_scale=0.0), "sigma_scale"),
    (dict(sigma_scale=-1.0), "sigma_scale"),
    (dict(sigma_scale=float("nan")), "sigma_scale"),
])
def test_bad_options_raise_before_the_device_check(kw, name):
    """A model on the CPU makes predict_per_patch raise Ru3dError ("lives on cpu"); a bad option is reported first."""
    image = np.zeros((8, 8, 8, 1), np.float32)
    with pytest.raises(ValueError, match=name):
        I.predict_per_patch(image, _cpu_model(), 2, (8, 8, 8), 2, False, **kw)
    with pytest.raises(ValueError, match=name):
        I.predict_case({"image": image, "affine": np.eye(4)}, _cpu_model(), (1, 1, 1), {}, 2, (8, 8, 8), 2, False, **kw)
    with pytest.raises(ValueError, match=name):
        I.Blended(_cpu_model(), **kw)


def test_bad_model_lists_raise_before_the_device_check():
    image = np.zeros((8, 8, 8, 1), np.float32)
    with pytest.raises(ValueError, match="model"):
        I.predict_per_patch(image, [], 2, (8, 8, 8), 2, False)
    with pytest.raises(ValueError, match="model"):
        I.predict_per_patch(image, (), 2, (8, 8, 8), 2, False, placement="cover")
    meta = _cpu_model().to("meta")
    with pytest.raises(ValueError, match="model.*different devices"):
        I.predict_per_patch(image, [_cpu_model(), meta], 2, (8, 8, 8), 2, False)
    # valid options: the next thing in the way is the device check
    for model in (_cpu_model(), [_cpu_model(), _cpu_model()], I.Blended([_cpu_model()], placement="cover", weighting="gaussian", mirror_axes=(0, 2), sigma_scale=0.25)):
        with pytest.raises(N.Ru3dError, match="lives on cpu"):
            I.predict_per_patch(image, model, 2, (8, 8, 8), 2, False, placement="cover", weighting="gaussian",
                                mirror_axes=(0, 2), sigma_scale=0.25)


def test_blended_carries_options_and_refuses_contradictions():
    m = _cpu_model(3)
    b = I.Blended([m, _cpu_model(3)], placement="cover", weighting="gaussian", mirror_axes=[2, 0])
    assert b.out_channels == 3 and next(b.parameters()) is next(m.parameters()) and len(b.models) == 2
    models, opt = I.resolve_options(b)
    assert models == b.models
    assert opt == dict(placement="cover", weighting="gaussian", mirror_axes=(2, 0), sigma_scale=0.125)
    assert I.resolve_options(b, placement="cover", mirror_axes=(2, 0))[1] == opt
    with pytest.raises(ValueError, match="sigma_scale"):
        I.resolve_options(b, placement="cover", sigma_scale=0.5)
    with pytest.raises(ValueError, match="mirror_axes"):
        I.resolve_options(b, mirror_axes=(1,))
    models, opt = I.resolve_options(m)
    assert models == [m] and opt == dict(placement="reference", weighting="uniform", mirror_axes=(), sigma_scale=0.125)
    with pytest.raises(ValueError, match="Blended"):
        I.Blended(b)


# --------------------------------------------------------------------------------------------------- interface
def test_keywords_and_reexports():
    assert T.predict_per_patch is I.predict_per_patch and T.predict_case is I.predict_case
    want = [("placement", "reference"), ("weighting", "uniform"), ("mirror_axes", ()), ("sigma_scale", 0.125)]
    for fn in (I.predict_per_patch, I.predict_case, T.batch_predict_case):
        p = inspect.signature(fn).parameters
        assert [(k, p[k].default) for k in list(p)[-4:]] == want
        assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(p)[-4:])
    p = inspect.signature(I.predict_per_patch).parameters
    assert list(p)[:9] == ["input", "model", "num_classes", "patch_size", "step_per_patch", "verbose", "one_hot",
                           "patch_batch", "return_device"]
    assert all(p[k].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for k in list(p)[:9])
    assert N.PREDICT_MAX_BATCH == 16
    for name in ("ru3d_predict_gather", "ru3d_predict_accumulate_weighted"):
        assert name in N.SIGNATURES and hasattr(N.lib, name)


def test_new_entry_points_refuse_bad_arguments_without_a_device():
    import ctypes
    fake = ctypes.c_void_p(4096)                                                # never dereferenced on these paths
    t = N.Tensor(4096, 2, 8, 8, 8, 3, 3, 0, 0)
    win = (ctypes.c_int32 * 8)(0, 0, 0, 0, 1, 0, 0, 7)
    lib = N.lib
    assert lib.ru3d_predict_accumulate_weighted(ctypes.byref(t), N.F32, 0, 0, None, None, None, fake, fake, 8, 8, 8, 1, 0, 0,
                                                None) < 0 and b"outside" in lib.ru3d_last_error()
    assert lib.ru3d_predict_accumulate_weighted(ctypes.byref(t), N.F32, 2, 0, None, None, None, fake, fake, 8, 8, 8, 0, 0, 0,
                                                None) < 0 and b"sample" in lib.ru3d_last_error()
    assert lib.ru3d_predict_accumulate_weighted(ctypes.byref(t), N.F32, 0, 8, None, None, None, fake, fake, 8, 8, 8, 0, 0, 0,
                                                None) < 0 and b"mirror" in lib.ru3d_last_error()
    assert lib.ru3d_predict_accumulate_weighted(ctypes.byref(t), N.F32, 0, 0, fake, None, fake, fake, fake, 8, 8, 8, 0, 0, 0,
                                                None) < 0 and b"tables" in lib.ru3d_last_error()
    assert lib.ru3d_predict_accumulate_weighted(ctypes.byref(t), N.F16, 0, 0, None, None, None, fake, fake, 8, 8, 8, 0, 0, 0,
                                                None) < 0 and b"dtype" in lib.ru3d_last_error()
    t9 = N.Tensor(4096, 1, 8, 8, 8, 9, 9, 0, 0)
    assert lib.ru3d_predict_accumulate_weighted(ctypes.byref(t9), N.F32, 0, 0, None, None, None, fake, fake, 8, 8, 8, 0, 0, 0,
                                                None) < 0 and b"classes" in lib.ru3d_last_error()
    x = N.Tensor(4096, 2, 8, 8, 8, 1, 1, 0, 0)
    assert lib.ru3d_predict_gather(fake, 8, 8, 8, 1, win, 2, ctypes.byref(x), None) < 0 and b"outside" in lib.ru3d_last_error()
    assert lib.ru3d_predict_gather(fake, 9, 8, 8, 1, win, 1, ctypes.byref(x), None) < 0 and b"batch" in lib.ru3d_last_error()
    big = N.Tensor(4096, 17, 8, 8, 8, 1, 1, 0, 0)
    wins = (ctypes.c_int32 * 68)()
    assert lib.ru3d_predict_gather(fake, 9, 8, 8, 1, wins, 17, ctypes.byref(big), None) < 0 and b"17 windows" in lib.ru3d_last_error()
    win[7] = 8
    win[4] = 0
    assert lib.ru3d_predict_gather(fake, 9, 8, 8, 1, win, 2, ctypes.byref(x), None) < 0 and b"mirror" in lib.ru3d_last_error()
