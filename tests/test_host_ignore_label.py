"""The ignore label of the softmax losses on the host: the torch twins loss._region_loss_host / loss._topk_loss_host
against the reference's numbers on the gathered voxels (fixture G14, tests/golden/make_golden_ignore.py) and against a
float64 restatement written here; the compaction identity (the loss with an ignore label is the plain loss of the counted
voxels gathered into one (1, C, M) batch); M = 0; the argument rules (ValueError, and the C entry points' refusals, all
before any launch); bad labels beside ignored ones; ignore_label=None; evaluation on numpy volumes against masked
bincounts; deep supervision with a level that reads only ignored labels; top-k with M < K.  No GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _native as N
import loss as L
import trainer as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = {"hybird": N.LOSS_HYBIRD, "diceloss": N.LOSS_DICELOSS, "focal": N.LOSS_FOCAL, "dice": N.LOSS_DICE}
ENTRY_POINTS = ["ru3d_loss_ignore_fwd", "ru3d_loss_ignore_bwd", "ru3d_ds_loss_ignore_fwd", "ru3d_ds_loss_ignore_bwd",
                "ru3d_topk_loss_ignore_fwd", "ru3d_topk_loss_ignore_bwd"]
G14_HYPER = {"hybird": dict(weight_v=[1, 10, 20], alpha=.9, beta=.1), "diceloss": {}, "focal": {}, "dice": {}}


def restated(kind, z, y, ig, gamma=2.0, weight_v=None, alpha=0.5, beta=0.5, smooth=1e-7):
    """The semantics of DESIGN.md section 25 in float64, class by class, nothing shared with the twin."""
    n, c = z.shape[0], z.shape[1]
    t = y.reshape(n, -1).long()
    keep = torch.ones_like(t, dtype=torch.bool) if ig is None else t != ig
    zz = torch.where(keep[:, None], z.double().reshape(n, c, -1), torch.zeros((), dtype=torch.float64))
    p, lp = torch.softmax(zz, 1), torch.log_softmax(zz, 1)
    m = max(int(keep.sum()), 1)
    w = torch.ones(c, dtype=torch.float64) if weight_v is None else torch.tensor(weight_v, dtype=torch.float64)
    w = w / w.abs().sum()
    total = 0.0
    for cls in range(c):
        k = keep.double()
        g = ((t == cls) & keep).double()
        pc = p[:, cls] * k
        tp, sp, sg = (pc * g).sum(), pc.sum(), g.sum()
        dice = (tp + smooth) / (tp + alpha * (sg - tp) + beta * (sp - tp) + smooth)
        focal = c * (-((1.0 - p[:, cls]) ** gamma) * g * lp[:, cls]).sum() / m
        total = total + w[cls] * {"hybird": 1.0 - dice + focal, "diceloss": 1.0 - dice, "focal": focal, "dice": dice}[kind]
    return total


def with_grad(fn, z):
    x = z.detach().clone().requires_grad_(True)
    v = fn(x)
    v.backward()
    return v.detach(), x.grad


def twin(kind, z, y, ig, gamma=2.0, weight_v=None, alpha=0.5, beta=0.5, smooth=1e-7):
    return with_grad(lambda x: L._region_loss_host(KINDS[kind], x, y, gamma, weight_v, alpha, beta, smooth, ig), z)


def draw(c, shape, seed, share=0.4, ig=255, dtype=torch.int64):
    g = torch.Generator().manual_seed(seed)
    z = 3 * torch.randn((shape[0], c) + tuple(shape[1:]), generator=g, dtype=torch.float64)
    y = torch.randint(0, c, tuple(shape), generator=g)
    y[torch.rand(tuple(shape), generator=g) < share] = ig
    return z, y.to(dtype)


@pytest.fixture(scope="module")
def g14(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "g14_ignore.npz")))


# --------------------------------------------------------------------------- the twin against the reference's numbers
@pytest.mark.parametrize("tag,labels", [("a", "y"), ("one", "y1")])
@pytest.mark.parametrize("kind", list(KINDS))
def test_twin_equals_the_reference_on_the_gathered_voxels(g14, tag, labels, kind):
    """The values were computed by the reference in float32: its per-class dices and focal means carry float32 rounding,
    a few 1e-7 on values of order 1 (9e-8 on 2.39 was measured on a 2 x 3 x 5 x 6 x 7 case), so 2e-6 absolute.  The gradients come from a
    float64 run of the reference, whose weights w = F.normalize(float32 weight_v) are float32 numbers: relative 2**-24
    = 6e-8 per weight, so 1e-6 of the largest gradient bounds the difference with room for nothing else."""
    z, y = torch.from_numpy(g14["z"]).double(), torch.from_numpy(g14[labels])
    v, g = twin(kind, z, y, 255, **G14_HYPER[kind])
    ref_v, ref_g = float(g14["%s/%s/value" % (tag, kind)]), torch.from_numpy(g14["%s/%s/grad" % (tag, kind)])
    assert abs(float(v) - ref_v) <= 2e-6, (float(v), ref_v)
    assert float((g - ref_g).abs().max()) <= 1e-6 * float(ref_g.abs().max())
    ignored = (y == 255)[:, None].expand_as(g)
    assert bool((g[ignored] == 0).all()) and bool((ref_g[ignored] == 0).all())


def test_g14_holds_the_patterns_it_is_meant_to(g14):
    y, y1 = g14["y"], g14["y1"]
    assert g14["z"].shape == (2, 3, 9, 10, 12) and g14["z"].dtype == np.float32 and y.dtype == np.uint8
    assert 0.35 < (y == 255).mean() < 0.45
    assert any(bool((y[:, k] == 255).all()) for k in range(9))          # one whole z-slab
    assert not (y[1] == 2).any() and (y[0] == 2).any()                  # class 2 of sample 1 only under ignored voxels
    assert int((y1 != 255).sum()) == 1
    assert set(np.unique(y)) == {0, 1, 2, 255}


# --------------------------------------------------------------------------- the twin against the restatement
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("c,ig,gamma", [(2, 255, 2.0), (3, -1, 1.5), (5, 255, 0.0), (8, 31, 1.0)])
def test_twin_equals_the_restatement(kind, c, ig, gamma):
    z, y = draw(c, (2, 5, 6, 7), seed=10 * c, ig=ig)
    hyper = dict(gamma=gamma, weight_v=[1.0 + 2 * k for k in range(c)], alpha=0.7, beta=0.3, smooth=1e-5)
    v, g = twin(kind, z, y, ig, **hyper)
    ref_v, ref_g = with_grad(lambda x: restated(kind, x, y, ig, **hyper), z)
    assert v.dtype == torch.float64
    assert abs(float(v) - float(ref_v)) <= 1e-12 * max(1.0, abs(float(ref_v)))
    assert float((g - ref_g).abs().max()) <= 1e-12 * max(float(ref_g.abs().max()), 1e-30)
    assert bool((g[(y == ig)[:, None].expand_as(g)] == 0).all())


@pytest.mark.parametrize("kind", list(KINDS))
def test_compaction_identity(kind):
    """The loss with an ignore label IS the plain loss of the counted voxels as one (1, C, M) batch."""
    c, ig = 3, 255
    z, y = draw(c, (2, 5, 6, 7), seed=3, ig=ig)
    hyper = dict(weight_v=[1, 10, 20], alpha=.9, beta=.1)
    v, g = twin(kind, z, y, ig, **hyper)
    keep = (y != ig).reshape(-1)
    rows = z.movedim(1, -1).reshape(-1, c)[keep]
    pv, pg = twin(kind, rows.t()[None].contiguous(), y.reshape(-1)[keep][None], None, **hyper)
    assert abs(float(v) - float(pv)) <= 1e-12
    back = torch.zeros(keep.numel(), c, dtype=torch.float64)
    back[keep] = pg[0].t()
    back = back.reshape(2, 5, 6, 7, c).movedim(-1, 1)
    assert float((g - back).abs().max()) <= 1e-12 * float(back.abs().max())


def test_logits_of_ignored_voxels_influence_nothing():
    z, y = draw(3, (2, 4, 5, 6), seed=4)
    hole = (y == 255)[:, None].expand_as(z)
    for poison in (float("nan"), float("inf"), -float("inf")):
        bad = z.clone()
        bad[hole] = poison
        zero = z.clone()
        zero[hole] = 0.0
        for kind in KINDS:
            v, g = twin(kind, bad, y, 255)
            v0, g0 = twin(kind, zero, y, 255)
            assert bool(torch.isfinite(v)) and float(v) == float(v0) and torch.equal(g, g0)
            assert bool((g[hole] == 0).all())
        tv, tg = with_grad(lambda x: L._topk_loss_host(x, y, 10, with_dice=True, ignore_label=255), bad)
        tv0, tg0 = with_grad(lambda x: L._topk_loss_host(x, y, 10, with_dice=True, ignore_label=255), zero)
        assert bool(torch.isfinite(tv)) and float(tv) == float(tv0) and torch.equal(tg, tg0) and bool((tg[hole] == 0).all())


# --------------------------------------------------------------------------- M = 0
def test_everything_ignored():
    z = 3 * torch.randn(2, 3, 4, 5, 6, dtype=torch.float64)
    y = torch.full((2, 4, 5, 6), 255)
    w = [1.0, 10.0, 20.0]
    for kind, want in (("hybird", 0.0), ("diceloss", 0.0), ("focal", 0.0), ("dice", 1.0)):      # Dice: sum w = 1
        v, g = twin(kind, z, y, 255, weight_v=w)
        assert float(v) == pytest.approx(want, abs=1e-15) and bool(torch.isfinite(v))
        assert bool((g == 0).all())
    for with_dice in (False, True):
        v, g = with_grad(lambda x: L._topk_loss_host(x, y, 10, with_dice=with_dice, ignore_label=255), z)
        assert float(v) == pytest.approx(0.0, abs=1e-15) and bool((g == 0).all())
    crit = L.DeepSupervisionLoss(L.HybirdLoss(ignore_label=255))
    v, g = with_grad(lambda x: crit([x], y), z)
    assert float(v) == pytest.approx(0.0, abs=1e-15) and bool((g == 0).all())


# --------------------------------------------------------------------------- argument rules
def test_constructors_keep_the_keyword():
    for cls in (L.Dice, L.DiceLoss, L.FocalLoss, L.HybirdLoss, L.TopKLoss, L.HybirdTopKLoss):
        assert cls().ignore_label is None
        assert cls(ignore_label=255).ignore_label == 255
        assert cls(ignore_label=-1).ignore_label == -1
    assert L.DeepSupervisionLoss(L.HybirdLoss(ignore_label=255)).ignore_label == 255
    assert L.DeepSupervisionLoss(L.FocalLoss()).ignore_label is None
    for cls in (L.SoftClDiceLoss, L.BoundaryLoss, L.DiceCoef, L.FocalDiceCoefLoss):
        with pytest.raises(TypeError):
            cls(ignore_label=255)
    with pytest.raises(TypeError):
        L.focal_loss(torch.zeros(4, 3), torch.zeros(4, dtype=torch.long), ignore_label=255)


@pytest.mark.parametrize("make", [lambda ig: L.Dice(ignore_label=ig), lambda ig: L.DiceLoss(ignore_label=ig),
                                  lambda ig: L.FocalLoss(ignore_label=ig), lambda ig: L.HybirdLoss(ignore_label=ig),
                                  lambda ig: L.TopKLoss(ignore_label=ig), lambda ig: L.HybirdTopKLoss(ignore_label=ig),
                                  lambda ig: L.DeepSupervisionLoss(L.HybirdLoss(ignore_label=ig))])
def test_value_errors_are_raised_per_call_before_anything_else(make):
    """Host tensors: the classes that only serve HIP tensors still answer the argument rules first."""
    x3, y3 = torch.zeros(1, 3, 4, 4, 4), torch.zeros(1, 4, 4, 4, dtype=torch.long)
    for ig in (0, 2):                                   # inside [0, C) of THIS call
        with pytest.raises(ValueError, match="class range"):
            make(ig)(x3, y3)
    with pytest.raises(ValueError, match="C == 1"):
        make(255)(torch.zeros(1, 1, 4, 4, 4), y3)
    for ig in (-1, 256):
        with pytest.raises(ValueError, match="uint8"):
            make(ig)(x3, y3.to(torch.uint8))
    # the same object is legal for a wider C ...
    crit = make(3)
    with pytest.raises(ValueError):
        crit(torch.zeros(1, 4, 4, 4, 4), y3)
    # ... and int64 labels take any int32 value outside [0, C)
    for ig in (-1, 255, 3):
        crit = make(ig)
        if isinstance(crit, (L.TopKLoss, L.HybirdTopKLoss, L.DeepSupervisionLoss)):
            assert bool(torch.isfinite(crit(x3, y3)))


def test_twins_apply_the_argument_rules():
    x, y = torch.zeros(1, 3, 8, dtype=torch.float64), torch.zeros(1, 8, dtype=torch.long)
    with pytest.raises(ValueError):
        L._region_loss_host(N.LOSS_HYBIRD, x, y, 2.0, None, .5, .5, 1e-7, 1)
    with pytest.raises(ValueError):
        L._region_loss_host(N.LOSS_HYBIRD, x[:, :1], y, 2.0, None, .5, .5, 1e-7, 255)
    with pytest.raises(ValueError):
        L._topk_loss_host(x, y.to(torch.uint8), 10, ignore_label=-1)
    with pytest.raises(ValueError):
        L._topk_loss_host(x, y, 10, ignore_label=2)


def test_entry_points_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "ru3d.h")).read()
    for name in ENTRY_POINTS:
        assert name + "(" in header and name in N.SIGNATURES and hasattr(N.lib, name)
    assert "max(M, 1)" in header and "ignore_label" in header


def test_c_abi_refuses_before_launch():
    fake = ctypes.c_void_p(4096)                        # never dereferenced: every call below is refused on its arguments
    big = 1 << 24

    def fwd(c=3, has=1, ig=255, label=N.LABEL_I64):
        return N.lib.ru3d_loss_ignore_fwd(fake, c * 100, 100, 1, fake, label, 2, 100, c, has, ig, N.LOSS_HYBIRD, 2.0, None,
                                          0.5, 0.5, 1e-7, fake, fake, fake, big, None)

    def bwd(c=3, has=1, ig=255, label=N.LABEL_I64):
        return N.lib.ru3d_loss_ignore_bwd(fake, c * 100, 100, 1, fake, label, 2, 100, c, has, ig, 2.0, fake, None, fake,
                                          N.F32, None)

    def tk_fwd(c=3, has=1, ig=255, label=N.LABEL_I64):
        return N.lib.ru3d_topk_loss_ignore_fwd(fake, c * 100, 100, 1, fake, label, 2, 100, c, has, ig, 20, 1, None, 0.5, 0.5,
                                               1e-7, 1.0, fake, fake, fake, fake, big, None)

    def tk_bwd(c=3, has=1, ig=255, label=N.LABEL_I64):
        return N.lib.ru3d_topk_loss_ignore_bwd(fake, c * 100, 100, 1, fake, label, 2, 100, c, has, ig, 1, fake, fake, None,
                                               fake, N.F32, None)

    level = (N.DsLevel * 1)(N.DsLevel(4096, 3 * 64, 64, 1, 4, 4, 4, 0))

    def ds_fwd(c=3, has=1, ig=255, label=N.LABEL_I64):
        return N.lib.ru3d_ds_loss_ignore_fwd(level, 1, fake, label, 2, 4, 4, 4, c, has, ig, N.LOSS_HYBIRD, 2.0, None, 0.5,
                                             0.5, 1e-7, fake, fake, fake, fake, big, None)

    def ds_bwd(c=3, has=1, ig=255, label=N.LABEL_I64):
        dptr = (ctypes.c_void_p * 1)(4096)
        return N.lib.ru3d_ds_loss_ignore_bwd(level, dptr, 1, fake, label, 2, 4, 4, 4, c, has, ig, 2.0, fake, None, None)

    for call in (fwd, bwd, tk_fwd, tk_bwd, ds_fwd, ds_bwd):
        for kw in (dict(ig=0), dict(ig=2), dict(c=1), dict(ig=-1, label=N.LABEL_U8), dict(ig=256, label=N.LABEL_U8),
                   dict(c=9), dict(label=7)):
            assert call(**kw) != 0, (call.__name__, kw)
            assert N.lib.ru3d_last_error()


# --------------------------------------------------------------------------- bad labels, ignore_label=None
def test_bad_labels_beside_ignored_ones_still_raise():
    z, y = draw(3, (2, 4, 5, 6), seed=6)
    for bad in (3, 7, -2, 254):
        yb = y.clone()
        yb[1, 2, 3, 4] = bad
        with pytest.raises(RuntimeError, match="Class values must be smaller than num_classes"):
            L._region_loss_host(N.LOSS_HYBIRD, z, yb, 2.0, None, .5, .5, 1e-7, 255)
        with pytest.raises(RuntimeError, match="Class values must be smaller than num_classes"):
            L._topk_loss_host(z, yb, 10, ignore_label=255)
        with pytest.raises(RuntimeError, match="Class values must be smaller than num_classes"):
            L.DeepSupervisionLoss(L.DiceLoss(ignore_label=255))([z], yb)
    with pytest.raises(RuntimeError):                   # without the keyword 255 is a bad label, as ever
        L._region_loss_host(N.LOSS_HYBIRD, z, y, 2.0, None, .5, .5, 1e-7)
    with pytest.raises(RuntimeError):
        L.TopKLoss()(z, y)


@pytest.mark.parametrize("kind", ["hybird", "diceloss", "focal"])
def test_none_is_the_former_twin(kind):
    """Without the keyword the twin runs its former statements: equal to the restatement without a mask, and - nothing
    ignored - the same bits as the call with an unused ignore label (the mask multiplies by 1.0, M is N V)."""
    z, y = draw(4, (2, 5, 6, 7), seed=8, share=0.0)
    hyper = dict(gamma=2.0, weight_v=[1, 2, 3, 4], alpha=.3, beta=.7)
    v, g = twin(kind, z, y, None, **hyper)
    ref_v, ref_g = with_grad(lambda x: restated(kind, x, y, None, **hyper), z)
    assert abs(float(v) - float(ref_v)) <= 1e-12 and float((g - ref_g).abs().max()) <= 1e-12 * float(ref_g.abs().max())
    v2, g2 = twin(kind, z, y, 255, **hyper)
    assert float(v2) == float(v) and torch.equal(g2, g)
    a = L._region_loss_host(KINDS[kind], z, y, 2.0, [1, 2, 3, 4], .3, .7, 1e-7)      # the former positional signature
    assert float(a) == float(v)
    tv = L._topk_loss_host(z, y, 10, True, [1, 2, 3, 4])
    assert float(tv) == float(L._topk_loss_host(z, y, 10, True, [1, 2, 3, 4], ignore_label=255))


# --------------------------------------------------------------------------- evaluation on numpy volumes
def masked_counts(pred, label, ig, c):
    keep = label != ig
    p, l = pred[keep].astype(np.int64), label[keep].astype(np.int64)
    k = int(max(p.max(), l.max())) + 1
    table = np.bincount(l * k + p, minlength=k * k).reshape(k, k)
    tp = int(table[c, c])
    fn, fp = int(table[c].sum()) - tp, int(table[:, c].sum()) - tp
    return tp, fn, fp, int(table.sum()) - tp - fn - fp


@pytest.mark.parametrize("ig,dtype", [(255, np.uint8), (-1, np.int64), (3, np.int16)])
def test_evaluation_on_numpy_volumes(ig, dtype):
    rng = np.random.default_rng(5)
    label = rng.integers(0, 3, size=(12, 11, 10)).astype(dtype)
    pred = rng.integers(0, 3, size=label.shape).astype(np.uint8)
    hole = rng.random(label.shape) < 0.3
    label[hole] = ig
    pred[3:5] = 2                                      # predictions under ignored voxels differ from anything else
    case = {"pred": pred, "label": label}
    dsc = T.evaluate_case(case, ignore_label=ig)
    met = T.evaluate_metrics(case, ignore_label=ig)
    assert len(dsc) == 2 and len(met) == 2
    total = int((~hole).sum())
    for c in (1, 2):
        tp, fn, fp, tn = masked_counts(pred, label, ig, c)
        assert tp + fn + fp + tn == total               # an ignored voxel is in no cell
        s = 1e-7
        assert dsc[c - 1] == pytest.approx((tp + s) / (tp + 0.5 * fn + 0.5 * fp + s), rel=1e-6)      # float32 loss.dice
        want = {"dsc": (tp + s) / (tp + 0.5 * (fn + fp) + s), "sen": (tp + s) / (tp + fn + s),
                "spe": (tn + s) / (tn + fp + s), "acc": (tp + tn + s) / (tp + tn + fn + fp + s)}
        assert met[c - 1] == want
    # the default changes nothing
    plain = {"pred": pred, "label": np.where(hole, 0, label).astype(np.uint8)}
    assert T.evaluate_metrics(plain) == T.evaluate_metrics(plain, ignore_label=None)
    assert T.evaluate_case(plain) == T.evaluate_case(plain, ignore_label=77)
    everything = {"pred": pred, "label": np.full(label.shape, ig).astype(dtype)}
    assert T.evaluate_case(everything, ignore_label=ig) == [] and T.evaluate_metrics(everything, ignore_label=ig) == []


# --------------------------------------------------------------------------- deep supervision
@pytest.mark.parametrize("kind,cls", [("hybird", L.HybirdLoss), ("diceloss", L.DiceLoss), ("focal", L.FocalLoss)])
def test_deep_supervision_with_a_level_of_ignored_labels_only(kind, cls):
    g = torch.Generator().manual_seed(12)
    full = (9, 10, 12)
    y = torch.randint(0, 3, (2,) + full, generator=g)
    y[torch.rand((2,) + full, generator=g) < 0.3] = 255
    y[:, ::4, ::4, ::4] = 255                          # all that level 2 reads: M_2 = 0
    assert int((y[:, ::2, ::2, ::2] != 255).sum()) > 0
    outs = [3 * torch.randn((2, 3) + tuple(-(-s // (1 << l)) for s in full), generator=g, dtype=torch.float64)
            for l in range(3)]
    crit = L.DeepSupervisionLoss(cls(weight_v=[1, 2, 3], ignore_label=255))
    xs = [o.clone().requires_grad_(True) for o in outs]
    total = crit(xs, y)
    total.backward()
    per = [restated(kind, o, L.downsample_labels(y, l), 255, weight_v=[1, 2, 3]) for l, o in enumerate(outs)]
    ws = L.deep_supervision_weights(3)
    assert abs(float(total.detach()) - sum(w * float(v) for w, v in zip(ws, per))) <= 1e-12
    got = crit.last_level_losses
    assert got.shape == (3,)
    for l in range(3):
        assert float(got[l]) == pytest.approx(float(per[l]), rel=1e-6, abs=1e-7)      # kept as float32
    assert float(per[2]) == pytest.approx(0.0, abs=1e-15) and bool((xs[2].grad == 0).all())
    for l in range(2):
        ref_g = with_grad(lambda x: restated(kind, x, L.downsample_labels(y, l), 255, weight_v=[1, 2, 3]), outs[l])[1]
        assert float((xs[l].grad - ws[l] * ref_g).abs().max()) <= 1e-12 * float(ref_g.abs().max())
        hole = (L.downsample_labels(y, l) == 255)[:, None].expand_as(xs[l].grad)
        assert bool((xs[l].grad[hole] == 0).all())


# --------------------------------------------------------------------------- top-k
def independent_topk(z, y, k, ig):
    """torch's own ignore_index and top-k in float64 (nnU-Net's rule): value and gradient."""
    x = z.detach().double().requires_grad_(True)
    ce = F.cross_entropy(x, y, ignore_index=ig, reduction="none").reshape(-1)
    kk = max(1, int(ce.numel() * k / 100))
    v = torch.topk(ce, kk).values.mean()
    v.backward()
    return float(v.detach()), x.grad, kk


@pytest.mark.parametrize("share,k", [(0.4, 10), (0.95, 10), (0.4, 100), (0.95, 100)])
@pytest.mark.parametrize("ig", [255, -1])
def test_topk_follows_the_ignore_index_rule(share, k, ig):
    """K counts ALL voxels.  share = 0.95 with k = 10: M < K, tau = 0 and the ignored voxels tie there - they are
    constants of the selection, so whichever of them torch.topk picks the gradient is the same, and the counted voxels
    with ce > 0 all lie above tau.  k = 100 selects every voxel: the mean over N V voxels of a ce that is 0 where ignored."""
    z, y = draw(3, (2, 6, 7, 8), seed=int(100 * share) + k, share=share, ig=ig)
    ref_v, ref_g, kk = independent_topk(z, y, k, ig)
    m = int((y != ig).sum())
    assert (m < kk) == (share > 0.9 or k == 100)
    v, g = with_grad(lambda x: L._topk_loss_host(x, y, k, ignore_label=ig), z)
    assert abs(float(v) - ref_v) <= 1e-13 * max(1.0, abs(ref_v))
    assert float((g - ref_g).abs().max()) <= 1e-13 * float(ref_g.abs().max())
    assert bool((g[(y == ig)[:, None].expand_as(g)] == 0).all())
    # the module on host tensors is the twin; the Dice leg is the region twin's
    x = z.clone().requires_grad_(True)
    mv = L.TopKLoss(k=k, ignore_label=ig)(x, y)
    mv.backward()
    assert float(mv.detach()) == float(v) and torch.equal(x.grad, g)
    hv = L.HybirdTopKLoss(k=k, weight_v=[1, 2, 3], ignore_label=ig)(z, y)
    want = float(v) + float(restated("diceloss", z, y, ig, weight_v=[1, 2, 3]))
    assert abs(float(hv) - want) <= 1e-12
    assert "not implemented" in L.TopKLoss.__doc__ and "not implemented" in L.HybirdTopKLoss.__doc__
