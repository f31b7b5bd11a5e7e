"""Blended sliding-window inference on the HIP path (inference.py: placement='cover', weighting='gaussian',
mirror_axes, model lists) against fixture G12 (tests/golden/g12_tta.npz: the reference's network in float64 under the
merge rule of inference.py, pinned to the CPU oracle by tests/test_host_inference_tta.py).  `-m gpu` only.

Tolerance of the probabilities: tol = 5e-6 + 2 * K * 2**-24.  5e-6 is the per-window bound tests/test_gpu_predict.py
holds the fp32 forward + softmax to, and a convex combination of windows cannot exceed it; K is the largest number of
(window, flip, model) terms any voxel receives, computed here from the placement; the second term bounds the fp32
rounding of K additions into the numerator and the denominator of values <= 1.  Masks must equal the fixture wherever
the fixture's top-2 margin (distance from 0.5 for one class) exceeds 2 * tol; the voxels excused that way must be
under 1 % of the volume, which is asserted on the fixture itself."""
import ctypes
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no HIP device", allow_module_level=True)

import _native as N  # noqa: E402
import inference as I  # noqa: E402
import network  # noqa: E402
import trainer as T  # noqa: E402
from oracle import unet_oracle as O  # noqa: E402

DEV = torch.device("cuda:0")
STEP = 2
CONFIGS = {                       # name: (weighting, mirror axes, number of weight sets)
    "cover_uniform": ("uniform", (), 1),
    "cover_gaussian": ("gaussian", (), 1),
    "cover_gaussian_m012": ("gaussian", (0, 1, 2), 1),
    "cover_gaussian_m02_ens": ("gaussian", (0, 2), 2),
}


def _case(golden_dir, tag):
    g6 = np.load(os.path.join(golden_dir, "g6_predict.npz"))
    g12 = np.load(os.path.join(golden_dir, "g12_tta.npz"))
    patch = tuple(int(v) for v in g6[tag + "/patch"])
    _, pool, feat, ncls = (int(v) for v in g6[tag + "/meta"])
    models = []
    for z, prefix in ((g6, tag + "/w/"), (g12, tag + "/w2/")):
        m = network.ResUnet3D(num_pool=pool, num_features=feat, in_channels=1, out_channels=ncls)
        m.load_state_dict({k[len(prefix):]: torch.from_numpy(z[k]) for k in z.files if k.startswith(prefix)}, strict=True)
        models.append(m.to(DEV))
    return g12, g6[tag + "/image"], patch, ncls, models


def _margin(prob):
    if prob.shape[-1] == 1:
        return np.abs(prob[..., 0] - 0.5)
    s = np.sort(prob, axis=-1)
    return s[..., -1] - s[..., -2]


def _most_terms(shape, patch, mirror_axes, models):
    full = I.padded_shape(shape, patch)
    hits = np.zeros(full, dtype=np.int64)
    for ox, oy, oz in I.cover_window_origins(full, patch, STEP)[0]:
        hits[ox:ox + patch[0], oy:oy + patch[1], oz:oz + patch[2]] += 1
    return int(hits.max()) * (2 ** len(mirror_axes)) * models


def _check_against_fixture(g12, tag, config, prob, mask, k):
    gp, gm = g12["%s/%s/prob" % (tag, config)], g12["%s/%s/mask" % (tag, config)]
    tol = 5e-6 + 2 * k * 2.0 ** -24
    excused = _margin(gp) <= 2 * tol
    assert excused.mean() < 0.01                                           # the cap, on the fixture alone
    assert prob.dtype == np.float32 and prob.shape == gp.shape
    assert not np.isnan(prob).any()
    err = float(np.abs(prob - gp).max())
    diff = mask != gm
    print("g12 %s/%s: K=%d tol=%.3g max|dprob|=%.3g, mask differs on %d voxels (%d excused by the margin rule)"
          % (tag, config, k, tol, err, int(diff.sum()), int(excused.sum())))
    assert err <= tol
    assert mask.dtype == np.uint8 and mask.shape == gm.shape
    assert not (diff & ~excused).any()


@pytest.mark.parametrize("tag", ["a", "b", "d"])
@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("patch_batch", [1, 3])
def test_blended_prediction_vs_fixture(golden_dir, tag, config, patch_batch):
    g12, image, patch, ncls, models = _case(golden_dir, tag)
    weighting, mirror_axes, count = CONFIGS[config]
    model = models[0] if count == 1 else models[:count]
    kw = dict(patch_batch=patch_batch, placement="cover", weighting=weighting, mirror_axes=mirror_axes)
    prob = T.predict_per_patch(image, model, ncls, patch, STEP, False, True, **kw)
    mask = T.predict_per_patch(image, model, ncls, patch, STEP, False, False, **kw)
    k = _most_terms(image.shape[:3], patch, mirror_axes, count)
    if config == "cover_gaussian_m012":
        assert k == {"a": 96, "b": 32, "d": 64}[tag]
    _check_against_fixture(g12, tag, config, prob, mask, k)


def test_defaults_are_untouched(golden_dir):
    """No new keyword, the defaults spelled out, and the plain model in a list: the same bits, NaN border included."""
    g12, image, patch, ncls, models = _case(golden_dir, "a")
    a = T.predict_per_patch(image, models[0], ncls, patch, 4, False, True)
    b = T.predict_per_patch(image, models[0], ncls, patch, 4, False, True, placement="reference", weighting="uniform",
                            mirror_axes=(), sigma_scale=0.125)
    c = T.predict_per_patch(image, [models[0]], ncls, patch, 4, False, True)
    assert np.isnan(a).any()                                               # the reference's uncovered border is there
    assert np.array_equal(a, b, equal_nan=True) and np.array_equal(a, c, equal_nan=True)
    g6 = np.load(os.path.join(golden_dir, "g6_predict.npz"))
    assert np.array_equal(np.isnan(a), np.isnan(g6["a/prob"]))


def test_patch_batch_is_bit_stable(golden_dir):
    g12, image, patch, ncls, models = _case(golden_dir, "a")
    kw = dict(placement="cover", weighting="gaussian", mirror_axes=(0, 1, 2))
    out = [T.predict_per_patch(image, models[0], ncls, patch, STEP, False, True, patch_batch=pb, **kw) for pb in (1, 3, 5)]
    assert np.array_equal(out[0], out[1]) and np.array_equal(out[0], out[2])
    big = T.predict_per_patch(image, models[0], ncls, patch, STEP, False, True, patch_batch=20, **kw)   # two gather launches
    assert np.array_equal(out[0], big)


def test_odd_pad_lands_on_the_input_grid(golden_dir):
    """Case b is 11 long on axis 0 under a 16 patch: padded by 3 in front, so 'cover' crops at 3.  A crop at the
    reference's 2 would shift the map by one voxel - the fixture tells them apart."""
    g12, image, patch, ncls, models = _case(golden_dir, "b")
    assert image.shape[0] == 11 and patch[0] == 16
    full = I.padded_shape(image.shape[:3], patch)
    assert I.pad_offset(image.shape[:3], full)[0] == 3 and I.crop_offset(image.shape[:3], full)[0] == 2
    prob = T.predict_per_patch(image, models[0], ncls, patch, STEP, False, True, placement="cover")
    gp = g12["b/cover_uniform/prob"]
    assert np.abs(prob - gp).max() <= 5e-6 + 2 * 4 * 2.0 ** -24
    assert np.abs(prob[1:] - gp[:-1]).max() > 1e-3 and np.abs(prob[:-1] - gp[1:]).max() > 1e-3


class _Pointwise(torch.nn.Module):
    """A stand-in model: per-voxel channels (x, -x, x / 2) of its input - no spatial mixing, so mirroring the input and
    mirroring the output back is the identity and only the plumbing is under test."""
    out_channels = 3

    def __init__(self):
        super().__init__()
        self.scale = torch.nn.Parameter(torch.tensor([1.0, -1.0, 0.5]))

    def forward(self, x):
        return x * self.scale.view(1, 3, 1, 1, 1)


def test_mirroring_is_invisible_to_a_pointwise_model():
    model = _Pointwise().to(DEV)
    image = O.synth_image((21, 19, 13, 1), 7).numpy()
    for weighting in ("uniform", "gaussian"):
        plain = T.predict_per_patch(image, model, 3, (16, 16, 8), 2, False, True, placement="cover", weighting=weighting)
        assert not np.isnan(plain).any()
        for axes in ((0,), (1,), (2,), (0, 2), (0, 1, 2)):
            got = T.predict_per_patch(image, model, 3, (16, 16, 8), 2, False, True, patch_batch=3, placement="cover",
                                      weighting=weighting, mirror_axes=axes)
            k = 12 * 2 ** len(axes)
            assert np.abs(got - plain).max() <= 2 * (k + 12) * 2.0 ** -24, (weighting, axes)   # both sides round
    # and a pointwise model reproduces softmax of the voxel itself: the windows sit where they should
    x = torch.from_numpy(image)
    want = torch.softmax(torch.cat((x, -x, 0.5 * x), dim=-1), dim=-1).numpy()
    assert np.abs(plain - want).max() <= 1e-6 + 2 * 12 * 2.0 ** -24


# --------------------------------------------------------------------------------------------------- the kernels alone
def test_gather_equals_torch_flip():
    rng = np.random.default_rng(11)
    for cin, (X, Y, Z), (px, py, pz) in ((1, (13, 11, 17), (8, 6, 10)), (2, (13, 11, 17), (8, 6, 10)),
                                         (1, (12, 10, 24), (8, 8, 16)), (2, (12, 10, 24), (8, 8, 16))):
        vol = torch.from_numpy(rng.standard_normal((X, Y, Z, cin)).astype(np.float32)).to(DEV)
        wins = [(int(rng.integers(0, X - px + 1)), int(rng.integers(0, Y - py + 1)), int(rng.integers(0, Z - pz + 1)), f)
                for f in range(8)] + [(X - px, Y - py, Z - pz, 5), (0, 0, 0, 2)]
        if Z == 24:                                                        # rows that qualify for the 16-byte path
            wins = [(a, b, 4 * (c // 4), f) for a, b, c, f in wins]
        x = N.new_act(len(wins), cin, px, py, pz, torch.float32, DEV)
        x.fill_(float("nan"))
        flat = (ctypes.c_int32 * (4 * len(wins)))(*[v for w in wins for v in w])
        d = N.desc(x)
        N.check(N.lib.ru3d_predict_gather(N.ptr(vol), X, Y, Z, cin, flat, len(wins), ctypes.byref(d), N.stream()), "gather")
        for i, (ox, oy, oz, f) in enumerate(wins):
            want = vol[ox:ox + px, oy:oy + py, oz:oz + pz].permute(3, 0, 1, 2)
            dims = [1 + a for a in range(3) if f >> a & 1]
            want = torch.flip(want, dims) if dims else want
            assert torch.equal(x[i], want), (cin, Z, i, f)
    # refused before launch: a window outside the volume, more than 16 entries, a batch that does not match
    vol = torch.zeros((8, 8, 8, 1), device=DEV)
    x = N.new_act(2, 1, 8, 8, 8, torch.float32, DEV)
    d = N.desc(x)
    bad = (ctypes.c_int32 * 8)(0, 0, 0, 0, 0, 1, 0, 0)
    assert N.lib.ru3d_predict_gather(N.ptr(vol), 8, 8, 8, 1, bad, 2, ctypes.byref(d), N.stream()) != 0
    assert b"outside" in N.lib.ru3d_last_error()
    assert N.lib.ru3d_predict_gather(N.ptr(vol), 8, 8, 8, 1, bad, 1, ctypes.byref(d), N.stream()) != 0
    x17 = N.new_act(17, 1, 8, 8, 8, torch.float32, DEV)
    d17 = N.desc(x17)
    many = (ctypes.c_int32 * 68)()
    assert N.lib.ru3d_predict_gather(N.ptr(vol), 8, 8, 8, 1, many, 17, ctypes.byref(d17), N.stream()) != 0
    assert b"17 windows" in N.lib.ru3d_last_error()


def test_accumulate_weighted_against_numpy():
    """Random logits, overlapping windows, 1-4 classes, f32 and bf16, with and without tables, all 8 mirror masks.
    Bound: T * 2**-23 with T the number of terms added (each term <= 1 carries a rounding of the softmax, of the weight
    product and of the sum)."""
    rng = np.random.default_rng(5)
    X, Y, Z = 13, 11, 17
    P = (8, 6, 10)
    wins = [((0, 0, 0), 0), ((3, 1, 5), 1), ((5, 5, 7), 2), ((3, 1, 5), 3), ((2, 3, 4), 4), ((5, 0, 0), 5),
            ((1, 2, 3), 6), ((4, 4, 6), 7)]
    tables = [rng.uniform(0.05, 1.0, p).astype(np.float32) for p in P]
    dtab = [torch.from_numpy(t).to(DEV) for t in tables]
    w3 = (tables[0][:, None, None].astype(np.float64) * tables[1][None, :, None]) * tables[2][None, None, :]
    for C in (1, 2, 3, 4):
        for dt in (torch.float32, torch.bfloat16):
            for weighted in (False, True):
                acc = torch.zeros((X, Y, Z, C), device=DEV)
                cnt = torch.zeros((X, Y, Z), device=DEV)
                racc, rcnt = np.zeros((X, Y, Z, C)), np.zeros((X, Y, Z))
                g = [N.ptr(t) for t in dtab] if weighted else [None, None, None]
                for (ox, oy, oz), f in wins:
                    z = torch.from_numpy(rng.standard_normal((2,) + P + (C,)).astype(np.float32) * 3).to(dt)
                    zd = z.to(DEV).permute(0, 4, 1, 2, 3)
                    d = N.desc(zd)
                    N.check(N.lib.ru3d_predict_accumulate_weighted(ctypes.byref(d), N.dtype_code(dt), 1, f, *g, N.ptr(acc),
                                                                   N.ptr(cnt), X, Y, Z, ox, oy, oz, N.stream()), "accw")
                    zz = z[1].double()
                    p = torch.sigmoid(zz) if C == 1 else torch.softmax(zz, dim=-1)
                    dims = [a for a in range(3) if f >> a & 1]
                    p = (torch.flip(p, dims) if dims else p).numpy()
                    w = w3 if weighted else np.ones(P)
                    sl = (slice(ox, ox + P[0]), slice(oy, oy + P[1]), slice(oz, oz + P[2]))
                    racc[sl] += p * w[..., None]
                    rcnt[sl] += w
                bound = len(wins) * 2.0 ** -23
                assert np.abs(acc.cpu().numpy() - racc).max() <= bound, (C, dt, weighted)
                assert np.abs(cnt.cpu().numpy() - rcnt).max() <= bound, (C, dt, weighted)
                if not weighted:
                    assert np.array_equal(cnt.cpu().numpy(), rcnt)
    # flip 0 without tables is ru3d_predict_accumulate, bit for bit
    z = torch.from_numpy(rng.standard_normal((1,) + P + (3,)).astype(np.float32)).to(DEV).permute(0, 4, 1, 2, 3)
    d = N.desc(z)
    a1, c1 = torch.zeros((X, Y, Z, 3), device=DEV), torch.zeros((X, Y, Z), device=DEV)
    a2, c2 = torch.zeros((X, Y, Z, 3), device=DEV), torch.zeros((X, Y, Z), device=DEV)
    for _ in range(2):
        N.check(N.lib.ru3d_predict_accumulate(ctypes.byref(d), N.F32, 0, N.ptr(a1), N.ptr(c1), X, Y, Z, 2, 1, 3, N.stream()))
        N.check(N.lib.ru3d_predict_accumulate_weighted(ctypes.byref(d), N.F32, 0, 0, None, None, None, N.ptr(a2), N.ptr(c2),
                                                       X, Y, Z, 2, 1, 3, N.stream()))
    assert torch.equal(a1, a2) and torch.equal(c1, c2)
    # refused before launch
    assert N.lib.ru3d_predict_accumulate_weighted(ctypes.byref(d), N.F32, 0, 0, None, None, None, N.ptr(a2), N.ptr(c2),
                                                  X, Y, Z, 6, 1, 3, N.stream()) != 0
    assert N.lib.ru3d_predict_accumulate_weighted(ctypes.byref(d), N.F32, 1, 0, None, None, None, N.ptr(a2), N.ptr(c2),
                                                  X, Y, Z, 0, 0, 0, N.stream()) != 0
    z9 = torch.zeros((1,) + P + (9,), device=DEV).permute(0, 4, 1, 2, 3)
    d9 = N.desc(z9)
    a9 = torch.zeros((X, Y, Z, 9), device=DEV)
    assert N.lib.ru3d_predict_accumulate_weighted(ctypes.byref(d9), N.F32, 0, 0, None, None, None, N.ptr(a9), N.ptr(c2),
                                                  X, Y, Z, 0, 0, 0, N.stream()) != 0
    assert b"classes" in N.lib.ru3d_last_error()
    assert torch.equal(a1, a2) and not a9.any()


# --------------------------------------------------------------------------------------------------- ensembles, drivers
def test_a_list_of_one_is_the_bare_model(golden_dir):
    g12, image, patch, ncls, models = _case(golden_dir, "a")
    kw = dict(placement="cover", weighting="gaussian", mirror_axes=(1,))
    a = T.predict_per_patch(image, models[0], ncls, patch, STEP, False, True, **kw)
    b = T.predict_per_patch(image, [models[0]], ncls, patch, STEP, False, True, **kw)
    c = T.predict_per_patch(image, I.Blended(models[0], **kw), ncls, patch, STEP, False, True)
    assert np.array_equal(a, b) and np.array_equal(a, c)


def _g9(golden_dir):
    z = np.load(os.path.join(golden_dir, "g9_cascade.npz"))
    coarse = network.ResUnet3D(num_pool=2, num_features=4, in_channels=1, out_channels=1)
    detail = network.ResUnet3D(num_pool=2, num_features=4, in_channels=1, out_channels=3)
    coarse.load_state_dict({k[len("coarse/w/"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("coarse/w/")}, strict=True)
    detail.load_state_dict({k[len("detail/w/"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("detail/w/")}, strict=True)
    stats = dict(zip(("mean", "std", "pct_00_5", "pct_99_5"), (float(v) for v in z["stats"])))
    args = dict(spacing=(tuple(z["params"][0]), tuple(z["params"][1])), stats=stats,
                patches=(tuple(int(v) for v in z["patches"][0]), tuple(int(v) for v in z["patches"][1])),
                step=int(z["scalars"][0]), threshold=int(z["scalars"][1]), padding=int(z["scalars"][2]))
    return z, coarse.to(DEV).eval(), detail.to(DEV).eval(), args


def test_predict_case_and_cascade_with_blending(golden_dir):
    """predict_case with cover + gaussian + one mirror axis predicts every voxel (the reference placement leaves NaN in
    the same map); the cascade takes the options on its model arguments (inference.Blended), its host route and its
    device route return the same mask, voxel for voxel, as tests/test_gpu_cascade_device.py asks of the plain cascade,
    and return_device keeps the mask in HBM."""
    import data
    z, coarse, detail, a = _g9(golden_dir)
    case = {"case_id": "g9", "image": z["image"], "affine": z["affine"]}
    kw = dict(placement="cover", weighting="gaussian", mirror_axes=(2,))
    ref = T.predict_case(dict(case), detail, a["spacing"][1], a["stats"], 3, a["patches"][1], a["step"], verbose=False,
                         one_hot=True)["pred"]
    got = T.predict_case(dict(case), detail, a["spacing"][1], a["stats"], 3, a["patches"][1], a["step"], verbose=False,
                         one_hot=True, **kw)["pred"]
    assert got.shape == ref.shape == z["image"].shape[:3] + (3,)
    assert np.isnan(ref).any() and not np.isnan(got).any()
    assert np.abs(got.sum(-1) - 1).max() < 1e-4
    dev = T.predict_case(dict(case), [detail, detail], a["spacing"][1], a["stats"], 3, a["patches"][1], a["step"],
                         verbose=False, one_hot=True, return_device=True, **kw)["pred"]
    assert dev.is_cuda and np.abs(dev.cpu().numpy() - got).max() <= 1e-6          # the same model twice: the same mean

    regions = data.regions_crop_case({**case, "pred": z["coarse_pred"]}, a["threshold"], a["padding"], "pred")
    assert len(regions) >= 2
    for region in regions:
        rp = T.predict_case(region, detail, a["spacing"][1], a["stats"], 3, a["patches"][1], a["step"], verbose=False,
                            one_hot=True, **kw)["pred"]
        assert rp.shape == region["image"].shape[:-1] + (3,) and not np.isnan(rp).any()

    bc, bd = I.Blended(coarse, **kw), I.Blended([detail], **kw)
    common = (a["spacing"][0], a["stats"], a["patches"][0])
    rest = (a["spacing"][1], a["stats"], a["patches"][1], 3, a["step"], a["threshold"], a["padding"])
    host = T.cascade_predict_case(dict(case), bc, *common, bd, *rest, verbose=False, on_device=False)["pred"]
    devc = T.cascade_predict_case(dict(case), bc, *common, bd, *rest, verbose=False, on_device=True, return_device=True)["pred"]
    assert torch.is_tensor(devc) and devc.is_cuda and devc.dtype == torch.uint8
    assert host.dtype == np.uint8 and host.shape == tuple(devc.shape) == z["image"].shape[:3]
    differing = int((host != devc.cpu().numpy()).sum())
    assert differing == 0, "%d voxels differ between the two routes" % differing
    assert host.max() >= 1
    plain = T.cascade_predict_case(dict(case), coarse, *common, detail, *rest, verbose=False, on_device=True)["pred"]
    assert plain.shape == host.shape


def test_config2_sized_run_in_bf16():
    """ResUnet3D(4,32,1,3), a 160x128x128 case, 128^3 windows, cover + gaussian: no NaN, probabilities sum to 1 within
    1e-5, and bf16 agrees with fp32 on > 99.9 % of the confident voxels (fp32 top-2 margin > 0.05), the rule of
    test_predict_config2_patch_bf16_vs_fp32_masks."""
    torch.manual_seed(0)
    model = network.ResUnet3D(4, 32, 1, 3).to(DEV)
    image = O.synth_image((160, 128, 128, 1), 99).numpy()
    out = {}
    for dt in (torch.float32, torch.bfloat16):
        network.set_compute_dtype(model, dt)
        out[dt] = T.predict_per_patch(image, model, 3, (128, 128, 128), 2, False, True, patch_batch=2, placement="cover",
                                      weighting="gaussian")
    p32, p16 = out[torch.float32], out[torch.bfloat16]
    assert p32.shape == (160, 128, 128, 3)
    assert not np.isnan(p32).any() and not np.isnan(p16).any()
    assert np.abs(p32.sum(-1) - 1).max() < 1e-5 and np.abs(p16.sum(-1) - 1).max() < 1e-5
    assert np.abs(p32 - p16).max() < 0.1
    sure = _margin(p32) > 0.05
    agree = (p32[sure].argmax(-1) == p16[sure].argmax(-1)).mean()
    print("bf16 vs fp32 (cover, gaussian): max prob diff %.4f, confident voxels %.3f, agreement there %.5f"
          % (np.abs(p32 - p16).max(), sure.mean(), agree))
    assert agree > 0.999, agree
