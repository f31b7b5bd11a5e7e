"""The ignore label of the softmax losses on a real MI355X: the ignore forms of the kernels in csrc/loss.hip, deepsup.hip
and topk.hip against float64 references on the host, the reference's own numbers (fixture G14), the captured training
step, the patch sampler's label_pad_cval = 255 and the evaluation with HIP operands.

Reference: the loss of the counted voxels alone (loss.py, section "ignore label") - softmax in
float64 on the float32 logits with zeros written where the label is ignored, the formulas of csrc/loss.hip's header
comment with every sum over the counted voxels and the focal mean over max(M, 1), the gradient by float64 autograd; the
scalars enter as the float32 values the kernel is handed.

Tolerances are VALUE_TOL, GRAD_REL and GRAD_FLOOR of tests/test_gpu_loss_kernels.py, because the arithmetic per counted
voxel is the same and the ignore form only leaves voxels out:
  * value: |err| <= 2e-6 * max(1, |ref|).  The per-voxel terms are float32 (relative error ~1e-7 each, of either sign),
    summed in float32 only within one thread and one wave and in float64 from there on.
  * gradient, element by element: |err| <= 2e-5 * |ref| + 1e-6 * max|ref|.  The floor is there because the kernel holds p
    as a float32: in dz_c = u_c - p_c sum_k u_k both terms carry a few 2^-24 of the coefficients, whatever is left of
    their difference; that file measured up to 4.7e-7 of max|ref| for this arithmetic done in float32 on the host, and
    1e-6 is twice that.
  * in addition the gradient at every ignored voxel is compared with `== 0`, in every class channel.
Top-k: the float64 twin loss._topk_loss_host, tie rule included.  As in tests/test_gpu_topk.py, selection next to the
threshold is where float32 and float64 may legitimately disagree: COUNTED voxels whose float64 ce lies within
1e-5 * max(1, tau) of the float64 tau are left out of the element-wise comparison (never of the value comparison, and an
ignored voxel is never left out of the `== 0` comparison); at most 4 may be left out.
Run with `-m gpu`."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no HIP device", allow_module_level=True)

import _native as N  # noqa: E402
import _ops as ops  # noqa: E402
import augment  # noqa: E402
import graph  # noqa: E402
import loss as L  # noqa: E402
import network  # noqa: E402
import optim  # noqa: E402
import trainer as T  # noqa: E402
import transform  # noqa: E402
from oracle import unet_oracle as O  # noqa: E402

DEV = torch.device("cuda:0")
KINDS = ["HybirdLoss", "DiceLoss", "FocalLoss", "Dice"]
KIND_CODE = {"HybirdLoss": N.LOSS_HYBIRD, "DiceLoss": N.LOSS_DICELOSS, "FocalLoss": N.LOSS_FOCAL, "Dice": N.LOSS_DICE}
G14_NAME = {"HybirdLoss": "hybird", "DiceLoss": "diceloss", "FocalLoss": "focal", "Dice": "dice"}
VALUE_TOL = 2e-6
GRAD_REL = 2e-5
GRAD_FLOOR = 1e-6
NEAR = 1e-5
MAX_LEFT_OUT = 4
BAD_LABELS = "Class values must be smaller than num_classes."


def f32(x):
    return float(torch.tensor(float(x), dtype=torch.float32))


def make(kind, ignore_label=None, gamma=2, weight_v=None, alpha=0.5, beta=0.5, smooth=1e-7):
    if kind == "HybirdLoss":
        return L.HybirdLoss(gamma=gamma, weight_v=weight_v, alpha=alpha, beta=beta, smooth=smooth, ignore_label=ignore_label)
    if kind == "DiceLoss":
        return L.DiceLoss(weight_v=weight_v, alpha=alpha, beta=beta, smooth=smooth, ignore_label=ignore_label)
    if kind == "FocalLoss":
        return L.FocalLoss(gamma=gamma, weight_v=weight_v, ignore_label=ignore_label)
    return L.Dice(weight_v=weight_v, alpha=alpha, beta=beta, smooth=smooth, ignore_label=ignore_label)


def run(kind, x, y, ig, upstream=None, **kw):
    """Value and gradient from the HIP kernels; x keeps its strides and its dtype."""
    x = x.detach().requires_grad_(True)
    v = make(kind, ig, **kw)(x, y)
    assert v.dim() == 0 and v.is_cuda and v.dtype == torch.float32
    (v if upstream is None else upstream(v)).backward()
    assert x.grad.shape == x.shape and x.grad.dtype == x.dtype
    return v.detach(), x.grad.detach()


def region_value(kind, z, y, ig, gamma=2, weight_v=None, alpha=0.5, beta=0.5, smooth=1e-7):
    """The float64 definition on host tensors (differentiable in z): sums over the counted voxels, focal over max(M, 1)."""
    n, c = z.shape[0], z.shape[1]
    yf = y.long().reshape(n, 1, -1)
    keep = yf != ig
    zf = torch.where(keep, z.reshape(n, c, -1), torch.zeros((), dtype=torch.float64))
    logp = torch.log_softmax(zf, dim=1)
    k = keep.to(torch.float64)
    p = logp.exp() * k
    safe = torch.where(keep, yf, torch.zeros_like(yf))
    g = torch.zeros(zf.shape, dtype=torch.float64).scatter_(1, safe, 1.0) * k
    w = torch.ones(c, dtype=torch.float64) if weight_v is None else torch.tensor([f32(a) for a in weight_v],
                                                                                 dtype=torch.float64)
    w = w / w.abs().sum().clamp_min(1e-12)
    a, b, s, gm = f32(alpha), f32(beta), f32(smooth), f32(gamma)
    tp, sp, sg = (p * g).sum((0, 2)), p.sum((0, 2)), g.sum((0, 2))
    dice = (tp + s) / (tp + a * (sg - tp) + b * (sp - tp) + s)
    lt = logp.gather(1, safe)
    per_voxel = (-((1.0 - lt.exp()) ** gm) * lt if gm != 0.0 else -lt) * k
    focal = torch.zeros(c, dtype=torch.float64).index_add(0, safe.reshape(-1), per_voxel.reshape(-1))
    focal = focal * c / max(int(keep.sum()), 1)
    return (w * {"HybirdLoss": 1.0 - dice + focal, "DiceLoss": 1.0 - dice, "FocalLoss": focal, "Dice": dice}[kind]).sum()


def reference(kind, x, y, ig, **kw):
    z = x.detach().to("cpu", torch.float64).contiguous().requires_grad_(True)
    v = region_value(kind, z, y.detach().cpu(), ig, **kw)
    v.backward()
    return float(v.detach()), z.grad


def assert_value(got, ref, what):
    got = float(got.detach()) if torch.is_tensor(got) else float(got)
    print("%s: value %.9g, float64 %.9g" % (what, got, ref))
    assert abs(got - ref) <= VALUE_TOL * max(1.0, abs(ref)), "%s: value %.9g, float64 %.9g" % (what, got, ref)


def assert_grad(got, ref, what, skip=None, unit=0.0):
    """unit: the unit roundoff of a 16-bit gradient (it is the float32 gradient rounded once)."""
    got = got.detach().to("cpu", torch.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), "%s: gradient not finite" % what
    err = (got - ref).abs()
    tol = (GRAD_REL + unit) * ref.abs() + GRAD_FLOOR * float(ref.abs().max())
    bad = err > tol
    if skip is not None:
        bad = bad & ~skip
    print("%s: worst gradient element at %.3g of its bound" % (what, float((err / tol.clamp_min(1e-300)).max())))
    assert not bool(bad.any()), "%s: %d gradient elements off, worst %.3g of its bound (max|ref| %.3g)" % (
        what, int(bad.sum()), float((err / tol.clamp_min(1e-300)).max()), float(ref.abs().max()))


def assert_zero_where_ignored(gx, y, ig, what):
    hole = (y == ig)[:, None].expand_as(gx)
    assert bool((gx[hole] == 0).all()), "%s: a gradient at an ignored voxel is not exactly 0" % what


def check(kind, x, y, ig, what, **kw):
    v, gx = run(kind, x, y, ig, **kw)
    ref_v, ref_g = reference(kind, x.float(), y, ig, **kw)
    assert_value(v, ref_v, what)
    assert_grad(gx, ref_g, what)
    assert_zero_where_ignored(gx, y, ig, what)
    return v, gx


def logits_and_labels(n, c, spatial, seed, share=0.4, ig=255, spread=2.0, label_dtype=torch.int64):
    g = torch.Generator().manual_seed(seed)
    x = spread * torch.randn((n, c) + tuple(spatial), generator=g)
    y = torch.randint(0, c, (n,) + tuple(spatial), generator=g)
    y[torch.rand((n,) + tuple(spatial), generator=g) < share] = ig
    return x.to(DEV), y.to(label_dtype).to(DEV)


# ------------------------------------------------------------------------------------------------ C x kind x layout
@pytest.mark.parametrize("layout", ["ncdhw", "ndhwc"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("c", [2, 3, 4, 5, 6, 7, 8])
def test_every_class_count_kind_and_layout(c, kind, layout):
    x, y = logits_and_labels(2, c, (5, 6, 7), 100 + c)
    if layout == "ndhwc":
        x = x.contiguous(memory_format=torch.channels_last_3d)
        assert not x.is_contiguous()
    _, gx = check(kind, x, y, 255, "%s C=%d %s" % (kind, c, layout))
    assert gx.stride() == x.stride()


# ------------------------------------------------------------------------------------------------ voxel counts
@pytest.mark.parametrize("nv", [1, 255, 2047, 2049, 999983])
def test_voxel_counts_around_the_reduction_layout(nv):
    """One thread, one short wave, either side of one workgroup's 2048 voxels, and a large odd count on which every
    forward workgroup strides."""
    x, y = logits_and_labels(1, 3, (nv,), 200 + nv % 97)
    if nv == 1:
        y[:] = 1                                       # the one voxel is counted (everything ignored is a case below)
    for kind in ("HybirdLoss", "Dice"):
        check(kind, x, y, 255, "%s N*V=%d" % (kind, nv))


# ------------------------------------------------------------------------------------------------ label types
def test_label_types_and_ignore_values():
    x, y = logits_and_labels(2, 4, (7, 9, 11), 31)
    hole = y == 255
    forms = [(y.to(torch.uint8), 255), (y, 255), (torch.where(hole, torch.full_like(y, -1), y), -1),
             (torch.where(hole, torch.full_like(y, 4), y), 4), (y.to(torch.int32), 255)]
    for kind in KINDS:
        first = None
        for lab, ig in forms:
            v, gx = check(kind, x, lab, ig, "%s %s ignore %d" % (kind, lab.dtype, ig))
            if first is None:
                first = (v, gx)
            assert torch.equal(v, first[0]) and torch.equal(gx, first[1])      # one mask, one result


# ------------------------------------------------------------------------------------------------ hyper-parameters
@pytest.mark.parametrize("gamma", [0, 1, 2, 1.5])
@pytest.mark.parametrize("kind", ["HybirdLoss", "FocalLoss"])
def test_focal_exponent_branches(gamma, kind):
    x, y = logits_and_labels(2, 3, (5, 6, 7), 41)
    check(kind, x, y, 255, "%s gamma=%g" % (kind, gamma), gamma=gamma)


@pytest.mark.parametrize("hyper", [dict(weight_v=[1, 10, 20]), dict(weight_v=[0.0, 1.0, -3.0]),
                                   dict(alpha=0.9, beta=0.1), dict(alpha=0.3, beta=0.7, smooth=1.0),
                                   dict(weight_v=[1, 10, 20], alpha=0.9, beta=0.1, smooth=1e-3)])
def test_weights_and_tversky_scalars(hyper):
    x, y = logits_and_labels(2, 3, (5, 6, 7), 51)
    for kind in KINDS:
        kw = {k: v for k, v in hyper.items() if kind != "FocalLoss" or k == "weight_v"}
        check(kind, x, y, 255, "%s %r" % (kind, kw), **kw)


def test_upstream_gradient():
    x, y = logits_and_labels(2, 3, (5, 6, 7), 81)
    for kind in ("HybirdLoss", "Dice"):
        _, g1 = run(kind, x, y, 255)
        _, g_big = run(kind, x, y, 255, upstream=lambda t: 65536.0 * t)
        _, g_neg = run(kind, x, y, 255, upstream=lambda t: -t)
        assert torch.equal(g_big, 65536.0 * g1) and torch.equal(g_neg, -g1)      # powers of two: exact
        _, g3 = run(kind, x, y, 255, upstream=lambda t: 3.0 * t + 1.0)
        assert_grad(g3, 3.0 * reference(kind, x, y, 255)[1], kind + ", 3 * loss + 1")
        assert_zero_where_ignored(g3, y, 255, kind)


@pytest.mark.parametrize("layout", ["ncdhw", "ndhwc"])
def test_bf16_logits(layout):
    """The kernels read float32: a bf16 tensor is up-cast first, so the value is the float32 call's on the up-cast
    tensor, bit for bit, and the gradient is that call's gradient rounded to bf16."""
    x, y = logits_and_labels(2, 3, (5, 6, 7), 71)
    x = x.to(torch.bfloat16)
    if layout == "ndhwc":
        x = x.contiguous(memory_format=torch.channels_last_3d)
    for kind in KINDS:
        v, gx = run(kind, x, y, 255)
        v32, g32 = run(kind, x.float(), y, 255)
        assert gx.dtype == torch.bfloat16 and torch.equal(v, v32) and torch.equal(gx, g32.to(torch.bfloat16)), kind
        ref_v, ref_g = reference(kind, x.float(), y, 255)
        assert_value(v, ref_v, "%s bf16" % kind)
        assert_grad(gx, ref_g, "%s bf16" % kind, unit=2.0 ** -8)
        assert_zero_where_ignored(gx, y, 255, kind)


# ------------------------------------------------------------------------------------------------ patterns
def test_nothing_ignored_is_the_plain_call_bit_for_bit():
    x, y = logits_and_labels(2, 4, (9, 10, 12), 61, share=0.0)
    for kind in KINDS:
        for kw in ({}, dict(weight_v=[1, 2, 3, 4], alpha=0.9, beta=0.1)):
            if kind == "FocalLoss":
                kw = {k: v for k, v in kw.items() if k == "weight_v"}
            v, gx = run(kind, x, y, 255, **kw)
            pv, pg = run(kind, x, y, None, **kw)
            assert torch.equal(v, pv) and torch.equal(gx, pg), kind
    for crit in (L.TopKLoss, L.HybirdTopKLoss):
        xa, xb = x.detach().requires_grad_(True), x.detach().requires_grad_(True)
        va, vb = crit(ignore_label=255)(xa, y), crit()(xb, y)
        va.backward()
        vb.backward()
        assert torch.equal(va, vb) and torch.equal(xa.grad, xb.grad)


def test_everything_ignored():
    """M = 0: dice_c = 1 for every class - DiceLoss, FocalLoss, HybirdLoss 0, Dice sum w = 1 -, finite, gradient == 0
    everywhere, and no error, neither now nor at the deferred label check."""
    x, _ = logits_and_labels(2, 3, (5, 6, 7), 62)
    for lab in (torch.full((2, 5, 6, 7), 255, dtype=torch.uint8, device=DEV),
                torch.full((2, 5, 6, 7), -1, dtype=torch.int64, device=DEV)):
        ig = int(lab.flatten()[0])
        for kind, want in (("HybirdLoss", 0.0), ("DiceLoss", 0.0), ("FocalLoss", 0.0), ("Dice", 1.0)):
            v, gx = run(kind, x, lab, ig, weight_v=[1, 10, 20])
            assert abs(float(v) - want) <= VALUE_TOL and bool((gx == 0).all()), (kind, float(v))
        for crit in (L.TopKLoss(ignore_label=ig), L.HybirdTopKLoss(ignore_label=ig)):
            xa = x.detach().requires_grad_(True)
            v = crit(xa, lab)
            v.backward()
            assert abs(float(v.detach())) <= VALUE_TOL and bool((xa.grad == 0).all())
    L.raise_on_bad_labels(wait=True)


def test_patterns_one_sample_one_class_one_voxel():
    x, y = logits_and_labels(2, 3, (5, 6, 7), 63, share=0.2)
    whole = y.clone()
    whole[1] = 255                                     # one whole sample ignored
    hidden = y.clone()
    hidden[y == 2] = 255                               # class 2 is present only under ignored voxels
    one = torch.full_like(y, 255)
    one[1, 4, 5, 6] = 2                                # M = 1: the very last voxel
    for name, lab in (("one sample ignored", whole), ("class 2 hidden", hidden), ("M = 1", one)):
        for kind in KINDS:
            check(kind, x, lab, 255, "%s, %s" % (kind, name), weight_v=[1, 10, 20])


@pytest.mark.parametrize("poison", [float("nan"), float("inf"), -float("inf")])
def test_non_finite_logits_at_ignored_voxels(poison):
    """The logits of an ignored voxel are never read: the loss and the other gradients equal the run with zeros there,
    bit for bit, and those voxels' gradient is == 0."""
    x, y = logits_and_labels(2, 3, (9, 10, 12), 64)
    hole = (y == 255)[:, None].expand_as(x)
    bad, zero = x.clone(), x.clone()
    bad[hole] = poison
    zero[hole] = 0.0
    for layout in ("ncdhw", "ndhwc"):
        if layout == "ndhwc":
            bad, zero = (t.contiguous(memory_format=torch.channels_last_3d) for t in (bad, zero))
        for kind in KINDS:
            v, gx = run(kind, bad, y, 255)
            v0, g0 = run(kind, zero, y, 255)
            assert bool(torch.isfinite(v)) and torch.equal(v, v0) and torch.equal(gx, g0), (kind, layout)
            assert_zero_where_ignored(gx, y, 255, kind)
        for crit in (L.TopKLoss(ignore_label=255), L.HybirdTopKLoss(ignore_label=255)):
            xa, xb = bad.detach().requires_grad_(True), zero.detach().requires_grad_(True)
            va, vb = crit(xa, y), crit(xb, y)
            va.backward()
            vb.backward()
            assert bool(torch.isfinite(va)) and torch.equal(va, vb) and torch.equal(xa.grad, xb.grad)
            assert_zero_where_ignored(xa.grad, y, 255, type(crit).__name__)
    crit = L.DeepSupervisionLoss(L.HybirdLoss(ignore_label=255))
    xa, xb = bad.detach().requires_grad_(True), zero.detach().requires_grad_(True)
    va, vb = crit([xa], y), crit([xb], y)
    va.backward()
    vb.backward()
    assert bool(torch.isfinite(va)) and torch.equal(va, vb) and torch.equal(xa.grad, xb.grad)


# ------------------------------------------------------------------------------------------------ G14
@pytest.fixture(scope="module")
def g14(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "g14_ignore.npz")))


@pytest.mark.parametrize("tag,labels", [("a", "y"), ("one", "y1")])
def test_g14_reference_numbers(g14, tag, labels):
    """The reference's own losses on the gathered (1, C, M) batch and their float64 gradients scattered back."""
    x, y = torch.from_numpy(g14["z"]).to(DEV), torch.from_numpy(g14[labels]).to(DEV)
    hyper = {"HybirdLoss": dict(weight_v=[1, 10, 20], alpha=.9, beta=.1)}
    for kind in KINDS:
        v, gx = run(kind, x, y, 255, **hyper.get(kind, {}))
        name = "%s/%s" % (tag, G14_NAME[kind])
        assert_value(v, float(g14[name + "/value"]), "G14 " + name)
        assert_grad(gx, torch.from_numpy(g14[name + "/grad"]), "G14 " + name)
        assert_zero_where_ignored(gx, y, 255, name)


# ------------------------------------------------------------------------------------------------ bad labels, refusals
def test_bad_label_next_to_ignored_ones():
    x, y = logits_and_labels(2, 3, (5, 6, 7), 65)
    y[0, 1, 2, 3] = 7
    L.raise_on_bad_labels(wait=True)
    for crit, args in ((L.HybirdLoss(ignore_label=255), x), (L.HybirdTopKLoss(ignore_label=255), x),
                       (L.DeepSupervisionLoss(L.DiceLoss(ignore_label=255)), [x])):
        v = crit(args, y)
        assert bool(torch.isnan(v)), type(crit).__name__             # counted by the kernel: NaN, the raise deferred
        with pytest.raises(RuntimeError, match=BAD_LABELS):
            L.raise_on_bad_labels(wait=True)
        crit.check_labels = True
        with pytest.raises(RuntimeError, match=BAD_LABELS):           # before the launch
            crit(args, y)
        good = y.clone()
        good[0, 1, 2, 3] = 255
        assert bool(torch.isfinite(crit(args, good)))                 # the blocking check skips the ignore value
    L.raise_on_bad_labels(wait=True)


def test_refusals_come_before_any_launch():
    """C == 1 and an ignore label inside the class range: ValueError from the modules, a non-zero status from the C entry
    points, and the state and output buffers still hold the pattern they were filled with."""
    for c, ig in ((1, 255), (3, 0), (3, 2)):
        x = torch.randn(2, c, 4, 4, 4, device=DEV)
        y = torch.zeros(2, 4, 4, 4, dtype=torch.int64, device=DEV)
        for kind in KINDS:
            with pytest.raises(ValueError):
                make(kind, ig)(x, y)
        with pytest.raises(ValueError):
            L.DeepSupervisionLoss(L.HybirdLoss(ignore_label=ig))([x], y)
        if c > 1:
            with pytest.raises(ValueError):
                L.HybirdTopKLoss(ignore_label=ig)(x, y)
        n, v = 2, 64
        state = torch.full((4096,), 0xAB, dtype=torch.uint8, device=DEV)
        out = torch.full((1,), 12345.0, device=DEV)
        ws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
        ce = torch.full((n * v,), 7.0, device=DEV)
        dz = torch.full_like(x, 9.0)
        block = torch.full((17,), 0.5, device=DEV)
        N.note_device(DEV)
        view = (N.ptr(x), c * v, v, 1, N.ptr(y), N.LABEL_I64, n)
        level = (N.DsLevel * 1)(N.DsLevel(x.data_ptr(), c * v, v, 1, 4, 4, 4, 0))
        dptr = (N.ctypes.c_void_p * 1)(dz.data_ptr())
        rcs = [N.lib.ru3d_loss_ignore_fwd(*view, v, c, 1, ig, N.LOSS_HYBIRD, 2.0, None, 0.5, 0.5, 1e-7, N.ptr(state),
                                          N.ptr(out), N.ptr(ws), ws.numel(), N.stream()),
               N.lib.ru3d_loss_ignore_bwd(*view, v, c, 1, ig, 2.0, N.ptr(state), None, N.ptr(dz), N.F32, N.stream()),
               N.lib.ru3d_ds_loss_ignore_fwd(level, 1, N.ptr(y), N.LABEL_I64, n, 4, 4, 4, c, 1, ig, N.LOSS_HYBIRD, 2.0, None,
                                             0.5, 0.5, 1e-7, N.ptr(block), N.ptr(state), N.ptr(out), N.ptr(ws), ws.numel(),
                                             N.stream()),
               N.lib.ru3d_ds_loss_ignore_bwd(level, dptr, 1, N.ptr(y), N.LABEL_I64, n, 4, 4, 4, c, 1, ig, 2.0, N.ptr(state),
                                             None, N.stream()),
               N.lib.ru3d_topk_loss_ignore_fwd(*view, v, c, 1, ig, 12, 1, None, 0.5, 0.5, 1e-7, 1.0, N.ptr(ce), N.ptr(state),
                                               N.ptr(out), N.ptr(ws), ws.numel(), N.stream()),
               N.lib.ru3d_topk_loss_ignore_bwd(*view, v, c, 1, ig, 1, N.ptr(ce), N.ptr(state), None, N.ptr(dz), N.F32,
                                               N.stream())]
        torch.cuda.synchronize()
        assert all(rc != 0 for rc in rcs), rcs
        assert bool((state == 0xAB).all()) and float(out) == 12345.0 and bool((dz == 9.0).all())
        assert bool((ce == 7.0).all()) and bool((block == 0.5).all())


# ------------------------------------------------------------------------------------------------ deep supervision
def _ds_reference(kind, outs, y, ig, weights, **kw):
    zs = [o.detach().to("cpu", torch.float64).contiguous().requires_grad_(True) for o in outs]
    per = [region_value(kind, z, L.downsample_labels(y.cpu(), l), ig, **kw) for l, z in enumerate(zs)]
    total = sum(w * v for w, v in zip(weights, per))
    total.backward()
    return float(total.detach()), [float(v.detach()) for v in per], [z.grad for z in zs]


@pytest.mark.parametrize("full,levels", [((9, 10, 12), 3), ((16, 16, 16), 4)])
@pytest.mark.parametrize("kind,cls", [("HybirdLoss", L.HybirdLoss), ("DiceLoss", L.DiceLoss), ("FocalLoss", L.FocalLoss)])
def test_deep_supervision(full, levels, kind, cls):
    """Level l reads target[:, ::2**l, ...] in place; the last level reads only ignored labels (M_l = 0: loss 0, gradient
    == 0), every level divides by its own max(M_l, 1); last_level_losses per level and one gradient per level."""
    g = torch.Generator().manual_seed(7 + levels)
    y = torch.randint(0, 3, (2,) + full, generator=g)
    y[torch.rand((2,) + full, generator=g) < 0.3] = 255
    step = 1 << (levels - 1)
    y[:, ::step, ::step, ::step] = 255
    assert int((y[:, ::step // 2, ::step // 2, ::step // 2] != 255).sum()) > 0
    y = y.to(torch.uint8 if levels == 3 else torch.int64).to(DEV)
    outs = [(2.0 * torch.randn((2, 3) + tuple(-(-s // (1 << l)) for s in full), generator=g)).to(DEV)
            for l in range(levels)]
    outs[1] = outs[1].contiguous(memory_format=torch.channels_last_3d)
    kw = dict(weight_v=[1, 10, 20])
    crit = L.DeepSupervisionLoss(cls(ignore_label=255, **kw))
    xs = [o.detach().requires_grad_(True) for o in outs]
    total = crit(xs, y)
    total.backward()
    ref_total, ref_per, ref_g = _ds_reference(kind, outs, y, 255, L.deep_supervision_weights(levels), **kw)
    assert_value(total, ref_total, "%s deep supervision %r" % (kind, full))
    got = crit.last_level_losses.cpu()
    for l in range(levels):
        assert_value(got[l], ref_per[l], "level %d" % l)
        if l < levels - 1:
            assert_grad(xs[l].grad, ref_g[l], "level %d" % l)
        assert_zero_where_ignored(xs[l].grad, L.downsample_labels(y, l), 255, "level %d" % l)
        assert xs[l].grad.stride() == xs[l].stride()
    assert float(got[levels - 1]) == 0.0 and ref_per[levels - 1] == 0.0 and bool((xs[levels - 1].grad == 0).all())


# ------------------------------------------------------------------------------------------------ top-k
@pytest.mark.parametrize("with_dice", [False, True], ids=["TopKLoss", "HybirdTopKLoss"])
@pytest.mark.parametrize("share,k", [(0.4, 10), (0.95, 10), (0.4, 100)])
@pytest.mark.parametrize("ig,label_dtype", [(255, torch.uint8), (-1, torch.int64)])
def test_topk(share, k, with_dice, ig, label_dtype):
    """k = 10 with 40 % ignored (tau > 0); k = 10 with 95 % ignored (M < K: tau = 0, the ignored voxels tie there and
    get nothing whatever share the rule gives); k = 100 (the mean over N V voxels of a ce that is 0 where ignored)."""
    x, y = logits_and_labels(2, 3, (9, 10, 12), 300 + k + int(100 * share), share=share, ig=ig, label_dtype=label_dtype)
    kw = dict(weight_v=[1, 10, 20], alpha=0.9, beta=0.1) if with_dice else {}
    crit = L.HybirdTopKLoss(k=k, ignore_label=ig, **kw) if with_dice else L.TopKLoss(k=k, ignore_label=ig)
    xa = x.detach().requires_grad_(True)
    v = crit(xa, y)
    v.backward()
    z = x.detach().to("cpu", torch.float64).requires_grad_(True)
    yc = y.cpu()
    f = {key: (f32(val) if not isinstance(val, list) else [f32(a) for a in val]) for key, val in kw.items()}
    ref = L._topk_loss_host(z, yc, k, with_dice=with_dice, smooth=f32(1e-7), ignore_label=ig, **f)
    ref.backward()
    kk = L.topk_count(y.numel(), k)
    m = int((yc != ig).sum())
    assert (m < kk) == (share > 0.9 or k == 100)
    what = "%s k=%g ignored %.2f" % (type(crit).__name__, k, share)
    assert_value(v, float(ref.detach()), what)
    # counted voxels whose float64 ce sits next to the float64 tau
    n, c = z.shape[0], z.shape[1]
    keep = (yc.long() != ig).reshape(n, -1)
    safe = torch.where(keep, yc.long().reshape(n, -1), torch.zeros((), dtype=torch.int64))
    ce = -torch.log_softmax(z.detach().reshape(n, c, -1), 1).gather(1, safe[:, None])[:, 0] * keep
    tau = float(torch.topk(ce.reshape(-1), kk).values[-1])
    near = ((ce - tau).abs() <= NEAR * max(1.0, tau)) & keep
    assert int(near.sum()) <= MAX_LEFT_OUT, "%d voxels next to the threshold" % int(near.sum())
    print("%s: tau %.6g, %d voxels left out" % (what, tau, int(near.sum())))
    skip = near.reshape(yc.shape)[:, None].expand_as(z)
    assert_grad(xa.grad, z.grad, what, skip=skip)
    assert_zero_where_ignored(xa.grad, y, ig, what)
    L.raise_on_bad_labels(wait=True)


# ------------------------------------------------------------------------------------------------ the captured step
def _step_batches(n):
    out = []
    for i in range(n):
        y = O.phantom_labels(1, (32, 32, 32), 3)
        y[:, 20 + i:26 + i] = 255                      # a slab nobody annotated, another one every step
        y[:, :, :, :3] = 255
        out.append((O.synth_image((1, 1, 32, 32, 32), 1700 + i).to(DEV), y.to(DEV)))
    return out


@pytest.mark.parametrize("deep", [False, True], ids=["HybirdLoss", "DeepSupervisionLoss"])
def test_captured_step_equals_the_eager_loop(deep):
    """One eager step and three replays through GraphedTrainStep leave the eager loop's losses and parameters, bit for
    bit, with labels that carry 255."""
    batches = _step_batches(4)
    assert int((batches[0][1] == 255).sum()) > 0 and int(batches[0][1][batches[0][1] != 255].max()) == 2

    def run_steps(graphed):
        torch.manual_seed(5)
        np.random.seed(5)
        ops._drop_counter[0] = 0
        model = network.ResUnet3D(2, 8, 1, 3, **(dict(deep_supervision=2) if deep else {})).to(DEV)
        model.train()
        opt = optim.Adam(model.parameters(), lr=1e-3)
        crit = L.HybirdLoss(ignore_label=255)
        if deep:
            crit = L.DeepSupervisionLoss(crit)
        step = graph.GraphedTrainStep(model, crit, opt, warmup=1) if graphed else None
        losses = []
        for x, y in batches:
            if graphed:
                losses.append(float(step(x, y)))
            else:
                opt.zero_grad(set_to_none=True)
                v = crit(model(x), y)
                v.backward()
                opt.step()
                losses.append(float(v.detach()))
        torch.cuda.synchronize()
        params = {k: v.clone() for k, v in model.state_dict().items()}
        if graphed:
            assert step.eager_steps == 1 and step.replays == 3
            L.raise_on_bad_labels(wait=True)
            step.release()
        return losses, params

    l_e, p_e = run_steps(False)
    l_g, p_g = run_steps(True)
    assert l_e == l_g, (l_e, l_g)
    assert all(np.isfinite(l_e)) and l_e[0] != l_e[1]
    bad = [k for k in p_e if not torch.equal(p_e[k], p_g[k])]
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ through the sampler
def _case_volume(block=False):
    shape = (24, 24, 16)
    rng = np.random.RandomState(11)
    g = np.meshgrid(*[np.linspace(-1, 1, s, dtype=np.float32) for s in shape], indexing="ij")
    img = (np.sin(4 * g[0]) * np.cos(3 * g[1]) + g[2] ** 2 + 0.05 * rng.randn(*shape)).astype(np.float32)[..., None]
    lab = np.zeros(shape, dtype=np.uint8)
    lab[np.sqrt(g[0] ** 2 + g[1] ** 2 + g[2] ** 2) < 0.8] = 1
    lab[np.sqrt((g[0] - 0.2) ** 2 + g[1] ** 2 + g[2] ** 2) < 0.35] = 2
    if block:
        lab[6:14, 8:18, 4:10] = 255                    # a region nobody annotated, stored in the case
    return img, lab


SAMPLER = dict(crop_size=16, rotation=0.5, label_pad_cval=255, scale=0.1)


def test_sampler_pads_with_the_ignore_label():
    """The patch of a rotated crop reaches outside the case: there the sampler writes label_pad_cval = 255, every label
    of the patch is a class or 255, and HybirdLoss(ignore_label=255) is finite with a zero gradient exactly there."""
    img, lab = _case_volume()
    case = augment.DeviceCase(img, lab, DEV)
    np.random.seed(3)
    aug = augment.DeviceAugment(mirror_p=None, contrast=None, brightness=None, gamma=None, crop_mode="random", **SAMPLER)
    _, patch = aug.sample(case)
    torch.cuda.synchronize()
    values = set(int(v) for v in patch.unique())
    assert values <= {0, 1, 2, 255} and 255 in values and len(values) > 1, values
    g = torch.Generator().manual_seed(1)
    x = (2.0 * torch.randn((1, 3) + tuple(patch.shape), generator=g)).to(DEV)
    y = patch[None]
    v, gx = check("HybirdLoss", x, y, 255, "HybirdLoss on a sampled patch")
    assert bool(torch.isfinite(v))
    hole = (y == 255)[:, None].expand_as(gx)
    assert bool((gx[~hole] != 0).any()) and bool((gx[hole] == 0).all())
    assert bool(((gx != 0).any(1) | (y == 255)).all())               # zero EXACTLY where the patch holds 255


def test_sampler_carries_a_stored_ignore_block_like_its_numpy_twin():
    img, lab = _case_volume(block=True)
    case = augment.DeviceCase(img, lab, DEV)
    np.random.seed(4)
    aug = augment.DeviceAugment(mirror_p=None, contrast=None, brightness=None, gamma=None, crop_mode="random", **SAMPLER)
    _, patch = aug.sample(case)
    torch.cuda.synchronize()
    got = patch.cpu().numpy()
    np.random.seed(4)
    twin = transform.RandomSpatialCrop(crop_size=[16, 16, 16], rotation=0.5, label_pad_cval=255, scale=0.1,
                                       crop_mode="random", label_margin=True)({"image": img.copy(), "label": lab.copy()})
    want, margin = twin["label"].astype(np.int64), twin["label_margin"]
    assert set(np.unique(got)) <= {0, 1, 2, 255} and (got == 255).any()
    differ = (got == 255) != (want == 255)
    # as tests/test_gpu_spatial.py: the two sides may only differ where the twin's vote is a tie in float64
    assert not (differ & (margin >= 1e-9)).any(), "%d voxels differ where the twin's decision is not a tie" % int(
        (differ & (margin >= 1e-9)).sum())
    assert int(differ.sum()) <= 8


# ------------------------------------------------------------------------------------------------ evaluation
@pytest.mark.parametrize("ig", [255, -1, 3])
@pytest.mark.parametrize("hip", ["both", "pred", "label"])
def test_evaluation_with_hip_operands_equals_the_numpy_route(ig, hip):
    rng = np.random.default_rng(9)
    label = rng.integers(0, 3, size=(20, 18, 16)).astype(np.int64)
    pred = rng.integers(0, 3, size=label.shape).astype(np.uint8)
    label[rng.random(label.shape) < 0.3] = ig
    pred[2:4] = 2
    host = {"pred": pred, "label": label}
    dev = {"pred": torch.from_numpy(pred).to(DEV) if hip != "label" else pred,
           "label": torch.from_numpy(label).to(DEV) if hip != "pred" else label}
    want = T.evaluate_metrics(host, ignore_label=ig)
    assert len(want) == 2
    assert T.evaluate_metrics(dev, ignore_label=ig) == want
    got = T.evaluate_case(dev, ignore_label=ig)
    assert got == [m["dsc"] for m in want]
    ref = T.evaluate_case(host, ignore_label=ig)                      # float32 loss.dice on the host
    assert all(abs(a - b) <= 1e-6 for a, b in zip(got, ref))
    if ig == 255:
        stray = label.copy()
        stray[5, 5, 5] = 40
        for case in ({"pred": dev["pred"], "label": torch.from_numpy(stray).to(DEV)},
                     {"pred": torch.from_numpy(pred).to(DEV), "label": stray}):
            with pytest.raises(ValueError, match="class above"):
                T.evaluate_metrics(case, ignore_label=255)
        with pytest.raises(ValueError, match="class above"):         # without the keyword 255 is such a class, as ever
            T.evaluate_metrics({"pred": torch.from_numpy(pred).to(DEV), "label": torch.from_numpy(label).to(DEV)})
