"""The fused loss kernels of csrc/loss.hip (softmax + focal + Tversky forward sums, finalize, backward; the functional
`dice`) against a float64 reference written here, on a real MI355X: every class count the kernels are instantiated for,
the branches of the focal exponent, voxel counts around the 256-thread / 2048-voxel layout of the reduction, strided
inputs, label types, weights, saturated logits, 16-bit inputs, the upstream gradient and the bf16 output of the C ABI.

Reference: softmax (sigmoid for C == 1) in float64 on the float32 logits, the formulas of the header comment of
csrc/loss.hip, the gradient by float64 autograd.

Tolerances (VALUE_TOL, GRAD_REL, GRAD_FLOOR below):
  * value: |err| <= 2e-6 * max(1, |ref|), the bound tests/test_gpu_parity.py::test_g3_losses holds.  The kernel's per-voxel
    terms are float32 (relative error ~1e-7 each, of either sign) and are summed in float32 only within one thread and
    one wave, in float64 from there on.
  * gradient, element by element: |err| <= 2e-5 * |ref| + GRAD_FLOOR * max|ref|.  Not a bound scaled by the largest
    element alone: an error confined to voxels with small gradients (a tail, a sample boundary) must not hide below
    it.  The floor is there because the kernel holds p as a float32: in dz_c = u_c - p_c sum_k u_k both terms carry a
    few 2^-24 of the coefficients qa, qb, qf (p itself comes out of expf with a relative error of 1e-7 .. 5e-7), whatever
    is left of their difference, and the largest gradient element is about a quarter of the largest coefficient
    (p (1 - p) <= 1/4).  2e-7 of max|ref|, the first guess, is exceeded by a factor of up to 2.4 by exactly this
    arithmetic done in float32 on the host (Dice and DiceLoss, where the two terms cancel most; 4.7e-7 of max|ref| at
    N * V = 999983); 1e-6 is twice that.
Run with `-m gpu`."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no HIP device", allow_module_level=True)

import _native as N  # noqa: E402
import loss as L  # noqa: E402
from oracle import unet_oracle as O  # noqa: E402

DEV = torch.device("cuda:0")
KINDS = ["HybirdLoss", "DiceLoss", "FocalLoss", "Dice"]
KIND_CODE = {"HybirdLoss": N.LOSS_HYBIRD, "DiceLoss": N.LOSS_DICELOSS, "FocalLoss": N.LOSS_FOCAL, "Dice": N.LOSS_DICE}
VALUE_TOL = 2e-6
GRAD_REL = 2e-5
GRAD_FLOOR = 1e-6


def f32(x):
    return float(torch.tensor(float(x), dtype=torch.float32))


def make(kind, gamma=2, weight_v=None, alpha=0.5, beta=0.5, smooth=1e-7):
    if kind == "HybirdLoss":
        return L.HybirdLoss(gamma=gamma, weight_v=weight_v, alpha=alpha, beta=beta, smooth=smooth)
    if kind == "DiceLoss":
        return L.DiceLoss(weight_v=weight_v, alpha=alpha, beta=beta, smooth=smooth)
    if kind == "FocalLoss":
        return L.FocalLoss(gamma=gamma, weight_v=weight_v)
    return L.Dice(weight_v=weight_v, alpha=alpha, beta=beta, smooth=smooth)


def run(kind, x, y, upstream=None, **kw):
    """Value and gradient from the HIP kernels; x keeps its strides and its dtype."""
    x = x.detach().requires_grad_(True)
    v = make(kind, **kw)(x, y)
    assert v.dim() == 0 and v.is_cuda and v.dtype == torch.float32
    (v if upstream is None else upstream(v)).backward()
    assert x.grad.shape == x.shape and x.grad.dtype == x.dtype
    return v.detach(), x.grad.detach()


def reference(kind, x, y, gamma=2, weight_v=None, alpha=0.5, beta=0.5, smooth=1e-7):
    """float64 value and gradient on the host; the scalars as the float32 values the kernel is handed."""
    z = x.detach().to("cpu", torch.float64).contiguous().requires_grad_(True)
    n, c = z.shape[0], z.shape[1]
    zf = z.reshape(n, c, -1)
    yf = y.detach().cpu().long().reshape(n, 1, -1)
    logp = torch.log_softmax(zf, dim=1) if c > 1 else torch.nn.functional.logsigmoid(zf)
    p = logp.exp()
    g = torch.zeros(zf.shape, dtype=torch.float64).scatter_(1, yf, 1.0)
    w = torch.ones(c, dtype=torch.float64) if weight_v is None else torch.tensor([f32(a) for a in weight_v],
                                                                                 dtype=torch.float64)
    w = w / w.abs().sum().clamp_min(1e-12)
    a, b, s, gm = f32(alpha), f32(beta), f32(smooth), f32(gamma)
    tp, sp, sg = (p * g).sum((0, 2)), p.sum((0, 2)), g.sum((0, 2))
    dice = (tp + s) / (tp + a * (sg - tp) + b * (sp - tp) + s)
    if kind in ("HybirdLoss", "FocalLoss"):
        # only the target class of a voxel contributes: gather it instead of multiplying by the one-hot tensor
        lt, pt = logp.gather(1, yf), p.gather(1, yf)
        per_voxel = -((1.0 - pt) ** gm) * lt if gm != 0.0 else -lt
        focal = torch.zeros(c, dtype=torch.float64).index_add(0, yf.reshape(-1), per_voxel.reshape(-1))
        focal = focal * c / (n * zf.shape[2])
    if kind == "HybirdLoss":
        v = (w * (1.0 - dice + focal)).sum()
    elif kind == "DiceLoss":
        v = (w * (1.0 - dice)).sum()
    elif kind == "FocalLoss":
        v = (w * focal).sum()
    else:
        v = (w * dice).sum()
    v.backward()
    return float(v.detach()), z.grad


def assert_value(got, ref, what):
    got = float(got)
    assert abs(got - ref) <= VALUE_TOL * max(1.0, abs(ref)), "%s: value %.9g, float64 %.9g" % (what, got, ref)


def assert_grad(got, ref, what, rel=GRAD_REL, floor=GRAD_FLOOR, scale=0.0):
    """scale: the size of the gradient on ordinary logits, for inputs on which every element of the true gradient is
    tiny (a perfect prediction): the float32 floor is relative to the coefficients, not to the gradient that remains."""
    got = got.detach().to("cpu", torch.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), "%s: gradient not finite" % what
    err = (got - ref).abs()
    tol = rel * ref.abs() + floor * max(float(ref.abs().max()), scale)
    bad = err > tol
    assert not bool(bad.any()), "%s: %d gradient elements off, worst %.3g of its bound (max|ref| %.3g)" % (
        what, int(bad.sum()), float((err / tol.clamp_min(1e-300)).max()), float(ref.abs().max()))


def check(kind, x, y, what, scale=0.0, **kw):
    v, gx = run(kind, x, y, **kw)
    ref_v, ref_g = reference(kind, x.float(), y, **kw)
    assert_value(v, ref_v, what)
    assert_grad(gx, ref_g, what, scale=scale)
    return v, gx


def logits_and_labels(n, c, spatial, seed, spread=2.0, label_dtype=torch.int64):
    g = torch.Generator().manual_seed(seed)
    x = spread * torch.randn((n, c) + tuple(spatial), generator=g)
    y = torch.randint(0, c, (n,) + tuple(spatial), generator=g).to(label_dtype)
    return x.to(DEV), y.to(DEV)


# ------------------------------------------------------------------------------------------------ C x kind x layout
@pytest.mark.parametrize("layout", ["ncdhw", "ndhwc"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("c", [1, 2, 3, 4, 5, 6, 7, 8])
def test_every_class_count_kind_and_layout(c, kind, layout):
    x, y = logits_and_labels(2, c, (5, 6, 7), 100 + c)
    if c == 1:
        y = torch.zeros_like(y)        # the reference's one-hot admits nothing else with one class (see below)
    if layout == "ndhwc":
        x = x.contiguous(memory_format=torch.channels_last_3d)
        assert c == 1 or not x.is_contiguous()
    _, gx = check(kind, x, y, "%s C=%d %s" % (kind, c, layout))
    assert gx.stride() == x.stride()
    if c > 1:
        # the oracle's restatement of the reference's loss.py as a second opinion on the reference written above
        oracle = {"HybirdLoss": O.hybird_loss, "DiceLoss": O.dice_loss, "FocalLoss": O.focal_loss,
                  "Dice": O.dice_metric}[kind]
        second = float(oracle(x.detach().cpu().double().contiguous(), y.cpu()))
        assert abs(reference(kind, x, y)[0] - second) <= 1e-7 * max(1.0, abs(second))     # its weights are float32


def test_one_class_takes_all_zero_targets_only():
    """C == 1: sigmoid, log(sigmoid(z)) for the focal term, and labels {0, 1} raise like the reference's F.one_hot."""
    x, _ = logits_and_labels(2, 1, (4, 5, 6), 7)
    y = torch.zeros((2, 4, 5, 6), dtype=torch.int64, device=DEV)
    y[1, 2, 3, 4] = 1
    for kind in KINDS:
        with pytest.raises(RuntimeError, match="Class values must be smaller than num_classes"):
            make(kind)(x, y)


# ------------------------------------------------------------------------------------------------ gamma branches
@pytest.mark.parametrize("kind", ["HybirdLoss", "FocalLoss"])
@pytest.mark.parametrize("gamma", [0, 1, 2, 3, 2.5, 0.5])
def test_focal_exponent_branches(gamma, kind):
    """pow_gamma's branches (0, 1, 2, powf) and the backward's (2, 0, powf).  Logits within +-6 of each other
    (spread 1.2, clamped): 1 - p >= 2e-3 stays far from 0, where (1 - p)^(gamma - 1) of a gamma < 1 has a pole that
    neither float32 nor the reference has a value for."""
    x, y = logits_and_labels(3, 3, (4, 5, 7), 31, spread=1.2)
    x = x.clamp(-3.0, 3.0)
    check(kind, x, y, "%s gamma=%s" % (kind, gamma), gamma=gamma)
    x2, y2 = logits_and_labels(2, 2, (3, 5, 4), 32, spread=1.2)
    check(kind, x2.clamp(-3.0, 3.0), y2, "%s gamma=%s C=2" % (kind, gamma), gamma=gamma)


# ------------------------------------------------------------------------------------------------ voxel counts
COUNTS = [(1, 1), (1, 255), (1, 256), (1, 257), (1, 2047), (1, 2049), (3, 85), (2, 128), (3, 683), (2, 1024),
          (1, 999983), (3, 333337), (2, 500001), (3, 1400003)]


@pytest.mark.parametrize("n,v", COUNTS)
def test_voxel_counts_around_the_reduction_layout(n, v):
    """N * V below, at and above one workgroup (256), one workgroup's eight voxels a thread (2048), a prime near 10^6,
    and 4.2e6 > 2048 * 256 * 8 where every thread of the capped grid loops more than eight times; N = 2, 3 with odd V
    puts the sample boundary of the i / V split inside a workgroup."""
    c = 2 if n * v > 10 ** 6 else 3
    x, y = logits_and_labels(n, c, (v,), 1000 + n * 7 + v % 1000)
    for kind in ("HybirdLoss", "Dice") if n * v > 10 ** 5 else KINDS:
        check(kind, x, y, "%s N=%d V=%d" % (kind, n, v))
    if n * v <= 2049:
        xt = x.permute(0, 2, 1).contiguous().permute(0, 2, 1)        # channels last: stride_v = C
        v1, g1 = run("HybirdLoss", xt, y)
        v0, g0 = run("HybirdLoss", x, y)
        assert torch.equal(v0, v1) and torch.equal(g0, g1)


@pytest.mark.parametrize("count", [1, 255, 256, 257, 2047, 2049, 999983, 2048 * 1024 + 3])
def test_functional_dice_at_ragged_counts(count):
    """ru3d_tversky: 1024 workgroups at most, 2048 elements a workgroup and round."""
    g = torch.Generator().manual_seed(count)
    p = torch.rand(count, generator=g)
    t = (torch.rand(count, generator=g) < 0.3).float()
    for alpha, beta in ((0.5, 0.5), (0.9, 0.1), (0.3, 0.4)):
        pd, td = p.double(), t.double()
        tp, fn, fp = (pd * td).sum(), ((1 - pd) * td).sum(), (pd * (1 - td)).sum()
        ref = float((tp + f32(1e-7)) / (tp + f32(alpha) * fn + f32(beta) * fp + f32(1e-7)))
        got = L.dice(p.to(DEV), t.to(DEV), alpha=alpha, beta=beta)
        assert got.is_cuda and got.dim() == 0
        assert abs(float(got) - ref) <= VALUE_TOL, (count, alpha, beta, float(got), ref)
    assert torch.equal(L.dice(p.to(DEV), t.to(DEV)), L.dice(p.to(DEV), t.to(DEV)))
    assert float(L.dice(p.to(DEV).view(1, -1), t.to(DEV).view(1, -1).long())) == float(L.dice(p.to(DEV), t.to(DEV)))


# ------------------------------------------------------------------------------------------------ strides
def test_channel_slice_of_a_wider_tensor():
    """stride_n = 7 V for C = 3: the batch stride is not C * V."""
    big, _ = logits_and_labels(2, 7, (4, 5, 6), 41)
    _, y = logits_and_labels(2, 3, (4, 5, 6), 42)
    x = big[:, 2:5]
    assert L._flat_strides(x) == (7 * 120, 120, 1) and not x.is_contiguous()
    for kind in KINDS:
        v, gx = check(kind, x, y, kind + " channel slice")
        v0, g0 = run(kind, x.contiguous(), y)
        assert torch.equal(v, v0) and torch.equal(gx, g0), kind
    # the same slice of a channels-last tensor: stride_c = 1, stride_v = 7
    xl = big.contiguous(memory_format=torch.channels_last_3d)[:, 2:5]
    assert L._flat_strides(xl) == (7 * 120, 1, 7)
    v, gx = check("HybirdLoss", xl, y, "channel slice, channels last")
    assert torch.equal(v, run("HybirdLoss", x.contiguous(), y)[0])


def test_spatial_slice_that_does_not_collapse():
    big, _ = logits_and_labels(2, 3, (6, 7, 9), 43)
    x = big[:, :, :, 1:5, 2:8]
    _, y = logits_and_labels(2, 3, (6, 4, 6), 44)
    assert L._flat_strides(x) is None
    for dtype in (torch.float32, torch.bfloat16):
        xs = big.to(dtype)[:, :, :, 1:5, 2:8]
        for kind in ("HybirdLoss", "Dice"):
            v, gx = run(kind, xs, y)
            v0, g0 = run(kind, xs.contiguous(), y)
            assert torch.equal(v, v0) and torch.equal(gx, g0), kind
            assert gx.shape == xs.shape and gx.dtype == dtype
    check("HybirdLoss", x, y, "spatial slice")


# ------------------------------------------------------------------------------------------------ labels, weights, scalars
def test_label_types_and_class_histograms():
    x, y = logits_and_labels(2, 4, (5, 6, 7), 51)
    v0, g0 = run("HybirdLoss", x, y)
    for dtype in (torch.uint8, torch.int32):
        v, gx = run("HybirdLoss", x, y.to(dtype))
        assert torch.equal(v, v0) and torch.equal(gx, g0), dtype
    # a class that never occurs (its dice is smooth / (beta fp + smooth)), and one class everywhere
    y3 = torch.where(y == 2, torch.zeros_like(y), y)
    for kind in KINDS:
        check(kind, x, y3, kind + ", class 2 absent")
        check(kind, x, torch.full_like(y, 3), kind + ", class 3 everywhere")


@pytest.mark.parametrize("weight_v", [[1, 0, 2, 0], [1, -2, 3, 0.5], [0, 0, 0, 0], None, [0, 0, 0, 5]],
                         ids=["zeros", "negative", "all_zero", "none", "one_class"])
def test_class_weights(weight_v):
    """w = weight_v / sum |weight_v| (F.normalize, p = 1: a negative entry stays negative, the norm is clamped at 1e-12);
    `weight_c` is accepted and has no effect (the reference's dead parameter)."""
    x, y = logits_and_labels(2, 4, (5, 6, 7), 52)
    for kind in KINDS:
        v, gx = check(kind, x, y, "%s weight_v=%s" % (kind, weight_v), weight_v=weight_v)
        if weight_v == [0, 0, 0, 0]:
            assert float(v) == 0.0 and float(gx.abs().max()) == 0.0
    with_c = L.HybirdLoss(weight_c=[9, 9, 9, 9], weight_v=weight_v)(x, y)
    assert torch.equal(with_c, L.HybirdLoss(weight_v=weight_v)(x, y))


@pytest.mark.parametrize("alpha,beta,smooth", [(0.3, 0.4, 1e-7), (0.9, 0.8, 1e-7), (0.0, 1.0, 1e-7), (0.5, 0.5, 0.0),
                                               (0.7, 0.3, 1.0)])
def test_tversky_scalars(alpha, beta, smooth):
    """alpha + beta != 1 (the A coefficient of the backward then has its (1 - alpha - beta) term) and smooth = 0 on a
    case where every class occurs, so no denominator vanishes."""
    x, y = logits_and_labels(2, 3, (5, 6, 7), 53)
    assert all(int((y == k).sum()) > 0 for k in range(3))
    for kind in ("HybirdLoss", "DiceLoss", "Dice"):
        check(kind, x, y, "%s a=%g b=%g s=%g" % (kind, alpha, beta, smooth), alpha=alpha, beta=beta, smooth=smooth)


# ------------------------------------------------------------------------------------------------ saturation
def _saturated(seed, c=3):
    x, y = logits_and_labels(2, c, (6, 6, 6), seed, spread=1.0)
    g = torch.Generator().manual_seed(seed + 1)
    hit = (torch.rand(y.shape, generator=g) < 0.2).to(DEV)
    up = torch.randint(0, c, y.shape, generator=g).to(DEV)
    down = (up + 1 + torch.randint(0, c - 1, y.shape, generator=g).to(DEV)) % c
    bump = torch.zeros_like(x)
    bump.scatter_(1, up[:, None], 80.0)
    bump.scatter_add_(1, down[:, None], torch.full_like(bump[:, :1], -80.0))
    return torch.where(hit[:, None], x + bump, x), y


@pytest.mark.parametrize("gamma", [2, 3, 1, 0])
@pytest.mark.parametrize("kind", ["HybirdLoss", "FocalLoss", "DiceLoss"])
def test_saturated_voxels(kind, gamma):
    """One class 80 above and one 80 below the rest on a fifth of the voxels: the losing class has p = e^-160, 0 in
    float32, and a log-probability of about -160 that must stay finite (the kernel takes it from the logits, not from
    log p); where that class is the target the focal term is 160."""
    x, y = _saturated(61)
    assert float((x.max(1).values - x.min(1).values).max()) > 150
    v, gx = check(kind, x, y, "%s gamma=%s saturated" % (kind, gamma), gamma=gamma)
    assert bool(torch.isfinite(v))


def test_degenerate_predictions():
    _, y = logits_and_labels(2, 4, (5, 6, 7), 62)
    onehot = torch.nn.functional.one_hot(y, 4).permute(0, 4, 1, 2, 3).float()
    ordinary, _ = logits_and_labels(2, 4, (5, 6, 7), 63)
    for what, x in (("all logits equal", torch.full((2, 4, 5, 6, 7), 0.37, device=DEV)),
                    ("perfect", 60.0 * onehot - 30.0),
                    ("perfectly wrong", -60.0 * onehot + 30.0)):
        for kind in KINDS:
            # a perfect prediction leaves a gradient of ~1e-26 everywhere: the floor is that of ordinary logits
            scale = float(reference(kind, ordinary, y)[1].abs().max())
            v, gx = check(kind, x, y, "%s, %s" % (kind, what), scale=scale)
    v, _ = run("HybirdLoss", 60.0 * onehot - 30.0, y)
    assert abs(float(v)) <= VALUE_TOL                 # dice 1, focal 0
    v, _ = run("Dice", 60.0 * onehot - 30.0, y)
    assert abs(float(v) - 1.0) <= VALUE_TOL


# ------------------------------------------------------------------------------------------------ 16-bit logits
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("layout", ["ncdhw", "ndhwc"])
def test_sixteen_bit_logits(dtype, layout):
    """The kernels read float32: a 16-bit tensor is up-cast first, so the value is the float32 call's on the up-cast
    tensor, bit for bit, and the gradient is that call's gradient rounded to the input's type."""
    x, y = logits_and_labels(2, 3, (5, 6, 7), 71)
    x = x.to(dtype)
    if layout == "ndhwc":
        x = x.contiguous(memory_format=torch.channels_last_3d)
    for kind in KINDS:
        v, gx = run(kind, x, y)
        v32, g32 = run(kind, x.float(), y)
        assert gx.dtype == dtype and gx.shape == x.shape
        assert torch.equal(v, v32), kind
        assert torch.equal(gx, g32.to(dtype)), kind
        assert_value(v, reference(kind, x.float(), y)[0], "%s %s" % (kind, dtype))


# ------------------------------------------------------------------------------------------------ upstream gradient
def test_upstream_gradient():
    x, y = logits_and_labels(2, 3, (5, 6, 7), 81)
    for kind in ("HybirdLoss", "Dice"):
        v, g1 = run(kind, x, y)
        _, g_big = run(kind, x, y, upstream=lambda t: 65536.0 * t)
        _, g_small = run(kind, x, y, upstream=lambda t: t * 2.0 ** -20)
        _, g_neg = run(kind, x, y, upstream=lambda t: -t)
        _, g_zero = run(kind, x, y, upstream=lambda t: 0.0 * t)
        assert torch.equal(g_big, 65536.0 * g1)                   # powers of two: exact
        assert torch.equal(g_small, g1 * 2.0 ** -20)
        assert torch.equal(g_neg, -g1)
        assert float(g_zero.abs().max()) == 0.0
        _, g3 = run(kind, x, y, upstream=lambda t: 3.0 * t + 1.0)
        ref_v, ref_g = reference(kind, x, y)
        assert_grad(g3, 3.0 * ref_g, kind + ", 3 * loss + 1")
    # two losses on one input accumulate
    xa = x.detach().requires_grad_(True)
    (L.DiceLoss()(xa, y) + L.FocalLoss()(xa, y)).backward()
    assert_grad(xa.grad, reference("HybirdLoss", x, y)[1], "DiceLoss + FocalLoss")


def test_same_input_same_bits():
    x, y = logits_and_labels(3, 4, (33, 35, 37), 91)
    for kind in KINDS:
        v1, g1 = run(kind, x, y)
        v2, g2 = run(kind, x, y)
        assert torch.equal(v1, v2) and torch.equal(g1, g2), kind


# ------------------------------------------------------------------------------------------------ C ABI: bf16 gradient
def _abi_fwd_bwd(x, y, c, kind, gamma, out_dtype, upstream=None):
    n, v = x.shape[0], x[0, 0].numel()
    st = L._flat_strides(x)
    # what production hands over is torch.empty: the forward initialises state, output and scratch itself
    state = torch.empty(N.lib.ru3d_loss_state_bytes(c), dtype=torch.uint8, device=DEV).fill_(0xFF)
    out = torch.full((), float("nan"), dtype=torch.float32, device=DEV)
    ws = torch.empty(N.lib.ru3d_loss_workspace_bytes(n, v, c), dtype=torch.uint8, device=DEV).fill_(0xFF)
    N.note_device(DEV)
    N.check(N.lib.ru3d_loss_fwd(N.ptr(x), st[0], st[1], st[2], N.ptr(y), N.LABEL_I64, n, v, c, KIND_CODE[kind],
                                float(gamma), None, 0.5, 0.5, 1e-7, N.ptr(state), N.ptr(out), N.ptr(ws), ws.numel(),
                                N.stream()), "loss_fwd")
    dz = torch.zeros_like(x, dtype=out_dtype)
    assert dz.stride() == x.stride()
    N.check(N.lib.ru3d_loss_bwd(N.ptr(x), st[0], st[1], st[2], N.ptr(y), N.LABEL_I64, n, v, c, float(gamma),
                                N.ptr(state), N.ptr(upstream) if upstream is not None else None, N.ptr(dz),
                                N.BF16 if out_dtype == torch.bfloat16 else N.F32, N.stream()), "loss_bwd")
    return out, dz


@pytest.mark.parametrize("layout", ["ncdhw", "ndhwc"])
@pytest.mark.parametrize("c", [1, 2, 5, 8])
def test_loss_bwd_writes_bf16_through_the_c_abi(c, layout):
    """dlogits_dtype == RU3D_BF16 is a form of ru3d_loss_bwd the Python module never asks for: element for element the
    float32 output rounded to nearest even."""
    x, y = logits_and_labels(2, c, (5, 6, 7), 95)
    if c == 1:
        y = torch.zeros_like(y)
    if layout == "ndhwc":
        x = x.contiguous(memory_format=torch.channels_last_3d)
    up = torch.tensor([3.0], device=DEV)
    for kind in ("HybirdLoss", "Dice"):
        for upstream in (None, up):
            v32, g32 = _abi_fwd_bwd(x, y, c, kind, 2.0, torch.float32, upstream)
            v16, g16 = _abi_fwd_bwd(x, y, c, kind, 2.0, torch.bfloat16, upstream)
            assert torch.equal(v32, v16)
            assert torch.equal(g16.view(torch.int16), g32.to(torch.bfloat16).view(torch.int16)), (kind, c)
            ref_v, ref_g = reference(kind, x, y)
            assert_value(v32, ref_v, "C ABI " + kind)
            assert_grad(g32, ref_g * (1.0 if upstream is None else 3.0), "C ABI " + kind)
            assert float(g16.float().abs().max()) > 0


# ------------------------------------------------------------------------------------------------ training size
def test_training_size_patch():
    """2 x 4 x 128^3, the shape the training step ends with: 4.2e6 voxels, every thread of the 2048 forward workgroups
    sums eight of them in float32 before the float64 part of the reduction."""
    x, y = logits_and_labels(2, 4, (128, 128, 128), 99, spread=1.5)
    x = x.contiguous(memory_format=torch.channels_last_3d)       # the network's output layout
    check("HybirdLoss", x, y, "HybirdLoss 2x4x128^3")
