"""The soft-clDice kernels of csrc/cldice.hip on a real MI355X: the soft skeleton (forward and gradient), the loss
modules SoftClDiceLoss and HybirdClDiceLoss (value and gradient down to the logits), sample and class isolation, the bit
equalities, the deferred label check and the captured training step.

Reference: the torch twin of the definition in loss.py (soft_skeleton / SoftClDiceLoss on host tensors), evaluated in
float64 on the float32 inputs, the gradient by float64 autograd; the Hybird part as in tests/test_gpu_loss_kernels.py.

The kernels' tile is (A, B, Z) = (8, 8, 32) voxels per workgroup (CD_TA, CD_TB, CD_TZ in cldice.hip); TILE_PLUS_ONE exceeds
it by one voxel on every axis.

Inputs of every gradient comparison keep float32 and float64 from choosing different extremal voxels: inside each
(sample, class) volume that enters the loss the probabilities are pairwise distinct by a wide margin (asserted in
float64 for every case: >= 6e-5 for C = 2, >= 1e-5 for C = 3; the C = 3 draws are seeded permutations of two grids of
probabilities - among 1080 independent values the smallest gap is near 1e-6 - and only classes 1 and 2 are ever
selected, so class 0 need not be separated).  Exact ties (copies of one minimum) are decided
by the same rule on both sides.  So no element is left out of any comparison.

Tolerances:
  * value: |err| <= 2e-6 * max(1, |ref|), the bound of the fused losses.
  * gradient, element by element: |err| <= 2e-5 * |ref| + F * max|ref|, F twice what the SAME chain evaluated in
    float32 on the host (the twin on .float() inputs, the Hybird part in float32 too) misses the float64 reference by,
    measured for each case on the host as the worst element error over max|ref| and rounded up to two digits:
        soft skeleton (2,3,12,10,9): k = 0: 1.02e-7, k = 1: 1.01e-7, k = 3: 9.08e-8, k = 64: 1.06e-7;
        (1,2,9,9,33) k = 3: 1.21e-7; (2,2,1,1,70): 5.74e-8; (1,2,2,1,1): 0 (each gradient is one upstream element);
        the strided view: 1.23e-7.
        losses: c2 soft ncdhw 5.86e-7, c2 hybird ndhwc u8 1.47e-7, c3 soft ndhwc 1.92e-7, c3 hybird ncdhw k1 2.16e-7,
        c3 soft classes=(2,) 9.72e-8, c3 hybird weighted 4.39e-7, c3 hybird tile+1 k0 2.26e-7, c2 soft line k64 1.62e-7,
        c2 hybird pair 9.46e-7, c3 hybird upstream 1024 2.38e-7, the bf16 case 2.7e-7 (the float32 gradient of the
        widened logits, which is what the floor is applied to; the bf16 gradient is that one rounded once).
  * skeleton values: see forward_bound.
    The floors stand next to the cases (SKEL_CASES, F_STRIDED, LOSS_CASES, F_BF16).
Run with `-m gpu`."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no HIP device", allow_module_level=True)

import loss as L  # noqa: E402
import network  # noqa: E402
import optim  # noqa: E402
import _ops as ops  # noqa: E402
from oracle import unet_oracle as O  # noqa: E402

DEV = torch.device("cuda:0")
VALUE_TOL = 2e-6
GRAD_REL = 2e-5
BASE = (2, 3, 12, 10, 9)
SMALL = (2, 2, 8, 7, 6)
TILE_PLUS_ONE = (1, 2, 9, 9, 33)
LINE = (2, 2, 1, 1, 70)
PAIR = (1, 2, 2, 1, 1)


# ------------------------------------------------------------------------------------------------ inputs
def distinct_probs(shape, seed):
    """float32 (N, K, A, B, Z), pairwise distinct inside each volume: a seeded permutation of a grid over (0.02, 0.98)."""
    n, k = shape[:2]
    v = int(np.prod(shape[2:]))
    g = torch.Generator().manual_seed(seed)
    vols = [torch.linspace(0.02, 0.98, v, dtype=torch.float64)[torch.randperm(v, generator=g)] for _ in range(n * k)]
    return torch.stack(vols).reshape(shape).float()


def smallest_gap(p):
    """Smallest difference between two values of one volume of (N, K, ...) float64 probabilities."""
    flat = p.reshape(p.shape[0] * p.shape[1], -1).sort(dim=1).values
    return float((flat[:, 1:] - flat[:, :-1]).min()) if flat.shape[1] > 1 else float("inf")


def logits_c2(shape_nabz, seed):
    """C = 2: the class margin is a seeded permutation of linspace(-4, 4, N * V)."""
    n = shape_nabz[0]
    v = int(np.prod(shape_nabz[1:]))
    g = torch.Generator().manual_seed(seed)
    m = torch.linspace(-4, 4, n * v, dtype=torch.float64)[torch.randperm(n * v, generator=g)].reshape(n, 1, v)
    base = torch.randn((n, 1, v), dtype=torch.float64, generator=g)
    x = torch.cat((base, base + m), 1).float().reshape((n, 2) + tuple(shape_nabz[1:]))
    y = torch.randint(0, 2, (n,) + tuple(shape_nabz[1:]), generator=g)
    return x, y


def logits_c2_bf16(shape_nabz, seed):
    """C = 2 in bfloat16: logit 1 a multiple of 1/4 in [-4, 4), logit 0 minus a multiple of 1/64 below 1/4 - both exact in
    bfloat16 - so the margins of a volume are distinct multiples of 1/64 (a seeded choice of the 512 there are)."""
    n = shape_nabz[0]
    v = int(np.prod(shape_nabz[1:]))
    assert v <= 512
    g = torch.Generator().manual_seed(seed)
    pick = torch.stack([torch.randperm(512, generator=g)[:v] for _ in range(n)])
    x = torch.stack((-(pick % 16).double() / 64, (pick // 16).double() / 4 - 4), 1).to(torch.bfloat16)
    y = torch.randint(0, 2, (n,) + tuple(shape_nabz[1:]), generator=g)
    return x.reshape((n, 2) + tuple(shape_nabz[1:])), y


def logits_c3(shape_nabz, seed):
    """C = 3: p_1 and p_2 are seeded permutations of two grids (steps 0.4 / V), p_0 the rest; the logits are log p plus a
    seeded shift per voxel."""
    n = shape_nabz[0]
    v = int(np.prod(shape_nabz[1:]))
    g = torch.Generator().manual_seed(seed)
    p1 = torch.stack([torch.linspace(0.03, 0.43, v, dtype=torch.float64)[torch.randperm(v, generator=g)] for _ in range(n)])
    p2 = torch.stack([torch.linspace(0.05, 0.45, v, dtype=torch.float64)[torch.randperm(v, generator=g)] for _ in range(n)])
    p = torch.stack((1 - p1 - p2, p1, p2), 1)
    x = (p.log() + torch.randn((n, 1, v), dtype=torch.float64, generator=g)).float()
    y = torch.randint(0, 3, (n,) + tuple(shape_nabz[1:]), generator=g)
    return x.reshape((n, 3) + tuple(shape_nabz[1:])), y


def assert_well_separated(x, classes, least):
    p = torch.softmax(x.double(), dim=1)[:, list(classes)]
    gap = smallest_gap(p)
    assert gap >= least, "input not separated: smallest gap %.3g" % gap


# ------------------------------------------------------------------------------------------------ comparisons
def assert_value(got, ref, what):
    got = float(got)
    print("%s: value %.9g, float64 %.9g, |err| %.3g" % (what, got, ref, abs(got - ref)))
    assert abs(got - ref) <= VALUE_TOL * max(1.0, abs(ref)), "%s: value %.9g, float64 %.9g" % (what, got, ref)


def assert_grad(got, ref, what, floor):
    got = got.detach().to("cpu", torch.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), "%s: gradient not finite" % what
    err = (got - ref).abs()
    top = float(ref.abs().max())
    print("%s: worst gradient error %.3g of max|ref| %.3g" % (what, float(err.max()) / max(top, 1e-300), top))
    tol = GRAD_REL * ref.abs() + floor * top
    bad = err > tol
    assert not bool(bad.any()), "%s: %d gradient elements off, worst %.3g of its bound (max|ref| %.3g)" % (
        what, int(bad.sum()), float((err / tol.clamp_min(1e-300)).max()), top)


# ------------------------------------------------------------------------------------------------ plane-level skeleton
def skeleton_reference(p, k, gout):
    x = p.detach().cpu().double().requires_grad_(True)
    s = L.soft_skeleton(x, iterations=k)
    s.backward(gout.double())
    return s.detach(), x.grad


def forward_bound(p, k):
    """Per voxel, what float32 may miss the float64 S_k by.  Inputs lie in [0, 1) and every x_j is a copy of input values,
    so D(x_{j+1}) is exact and d_j = 0 holds in both precisions at once; at such a level s_j = s_{j-1} exactly.  At
    a level with d_j > 0 there are four roundings of values in [0, 1] - the difference d_j, the product s d, the
    difference d - s d, the sum - each at most half a unit, 2^-25, and the recurrence does not amplify what it carries
    (ds_j/ds_{j-1} = 1 - d_j, ds_j/dd_j = 1 - s_{j-1}, both in [0, 1]).  So: 2^-23 times the number of levels j <= k with
    d_j[v] > 0, and exact equality where there is none."""
    xj = p.detach().cpu().double()
    levels = torch.zeros_like(xj)
    for _ in range(k + 1):
        xn = L.soft_erode(xj)
        levels += (xj - L.soft_dilate(xn) > 0).double()
        xj = xn
    return levels * 2.0 ** -23


def assert_forward(s, ref_s, bound, what):
    err = (s.detach().cpu().double() - ref_s).abs()
    print("%s: worst forward error %.3g, bound at most %.3g (%d levels)" % (
        what, float(err.max()), float(bound.max()), int(round(float(bound.max()) * 2.0 ** 23))))
    assert bool((err <= bound).all()), "%s: %d skeleton values off" % (what, int((err > bound).sum()))


def skeleton_device(p, k, gout):
    x = p.detach().to(DEV).requires_grad_(True)
    s = L.soft_skeleton(x, iterations=k)
    assert s.is_cuda and s.dtype == torch.float32 and s.shape == x.shape
    s.backward(gout.to(DEV))
    return s.detach(), x.grad.detach()


# (shape, k, F)
SKEL_CASES = [(BASE, 0, 2.1e-7), (BASE, 1, 2.1e-7), (BASE, 3, 1.9e-7), (BASE, 64, 2.2e-7), (TILE_PLUS_ONE, 3, 2.5e-7),
              (LINE, 3, 1.2e-7), (PAIR, 3, 0.0)]
F_STRIDED = 2.5e-7


@pytest.mark.parametrize("shape,k,floor", SKEL_CASES)
def test_soft_skeleton_forward_and_gradient(shape, k, floor):
    p = distinct_probs(shape, 101 + k)
    gout = torch.randn(shape, generator=torch.Generator().manual_seed(7))
    ref_s, ref_g = skeleton_reference(p, k, gout)
    s, g = skeleton_device(p, k, gout)
    what = "skeleton %s k=%d" % (shape, k)
    assert_forward(s, ref_s, forward_bound(p, k), what)
    assert_grad(g, ref_g, what, floor)


def test_soft_skeleton_strided_view():
    big = distinct_probs((2, 3, 12, 10, 18), 131)
    view = big[..., ::2]                       # Z stride 2: not contiguous
    assert not view.is_contiguous()
    gout = torch.randn(view.shape, generator=torch.Generator().manual_seed(9))
    ref_s, ref_g = skeleton_reference(view, 3, gout)
    xb = big.to(DEV).requires_grad_(True)
    s = L.soft_skeleton(xb[..., ::2], iterations=3)
    s.backward(gout.to(DEV))
    assert_forward(s, ref_s, forward_bound(view, 3), "strided view")
    assert_grad(xb.grad[..., ::2], ref_g, "strided view", F_STRIDED)
    assert float(xb.grad[..., 1::2].abs().max()) == 0.0


def test_samples_and_classes_are_isolated():
    for shape, k in ((BASE, 3), (TILE_PLUS_ONE, 2), (LINE, 3)):
        p = distinct_probs(shape, 151)
        gout = torch.randn(shape, generator=torch.Generator().manual_seed(13))
        s, g = skeleton_device(p, k, gout)
        for n in range(shape[0]):
            for c in range(shape[1]):
                s1, g1 = skeleton_device(p[n:n + 1, c:c + 1], k, gout[n:n + 1, c:c + 1])
                assert torch.equal(s[n:n + 1, c:c + 1], s1) and torch.equal(g[n:n + 1, c:c + 1], g1), (shape, n, c)


def test_binary_volume_on_the_device():
    """S_k of a {0, 1} volume through the float kernels (what the loss does for the labels): exact."""
    g = (torch.rand((2, 2, 12, 10, 9), generator=torch.Generator().manual_seed(3)) < 0.3).float()
    for k in (0, 3):
        assert torch.equal(L.soft_skeleton(g.to(DEV), iterations=k).cpu(), L.soft_skeleton(g, iterations=k))


# ------------------------------------------------------------------------------------------------ logit-level losses
def hybird_reference(z, y, weight_v=None):
    """HybirdLoss(gamma=2, alpha=beta=0.5, smooth=1e-7) in the dtype of z (tests/test_gpu_loss_kernels.py)."""
    n, c = z.shape[:2]
    zf = z.reshape(n, c, -1)
    yf = y.reshape(n, 1, -1)
    logp = torch.log_softmax(zf, dim=1)
    p = logp.exp()
    g = torch.zeros_like(zf).scatter_(1, yf, 1.0)
    w = torch.ones(c, dtype=z.dtype) if weight_v is None else torch.tensor(
        [float(torch.tensor(float(a), dtype=torch.float32)) for a in weight_v], dtype=z.dtype)
    w = w / w.abs().sum().clamp_min(1e-12)
    s = float(torch.tensor(1e-7, dtype=torch.float32))
    tp, sp, sg = (p * g).sum((0, 2)), p.sum((0, 2)), g.sum((0, 2))
    dice = (tp + s) / (tp + 0.5 * (sg - tp) + 0.5 * (sp - tp) + s)
    lt, pt = logp.gather(1, yf), p.gather(1, yf)
    focal = torch.zeros(c, dtype=z.dtype).index_add(0, yf.reshape(-1), (-((1.0 - pt) ** 2) * lt).reshape(-1))
    return (w * (1.0 - dice + focal * c / (n * zf.shape[2]))).sum()


def loss_reference(x, y, cl_weight, k, classes=None, weight_v=None, smooth=1.0, upstream=1.0, dtype=torch.float64):
    """Value and gradient by autograd through the twin, in `dtype`, on the host."""
    z = x.detach().cpu().float().to(dtype).contiguous().requires_grad_(True)
    yl = y.detach().cpu().long()
    cl = L.SoftClDiceLoss(iterations=k, weight_v=weight_v, classes=classes, smooth=smooth)(z, yl)
    v = cl if cl_weight is None else (1.0 - cl_weight) * hybird_reference(z, yl, weight_v) + cl_weight * cl
    (upstream * v).backward()
    return float(v.detach()), z.grad


def loss_device(x, y, cl_weight, k, classes=None, weight_v=None, smooth=1.0, upstream=1.0):
    x = x.detach().requires_grad_(True)
    if cl_weight is None:
        crit = L.SoftClDiceLoss(iterations=k, weight_v=weight_v, classes=classes, smooth=smooth)
    else:
        crit = L.HybirdClDiceLoss(cl_weight=cl_weight, iterations=k, classes=classes, cl_smooth=smooth, weight_v=weight_v)
    v = crit(x, y)
    assert v.dim() == 0 and v.is_cuda and v.dtype == torch.float32
    (v * upstream).backward()
    assert x.grad.shape == x.shape and x.grad.dtype == x.dtype and x.grad.stride() == x.stride()
    return v.detach(), x.grad.detach()


def make_case(name):
    """name -> (logits on the device in the case's layout / dtype, labels, keyword arguments, classes that enter)."""
    if name == "c2 soft ncdhw":
        x, y = logits_c2((2,) + BASE[2:], 201)
        return x, y, dict(cl_weight=None, k=3), (1,)
    if name == "c2 hybird ndhwc u8":
        x, y = logits_c2((2,) + BASE[2:], 203)
        return x.contiguous(memory_format=torch.channels_last_3d), y.to(torch.uint8), dict(cl_weight=0.5, k=3), (1,)
    if name == "c3 soft ndhwc":
        x, y = logits_c3((2,) + BASE[2:], 205)
        return x.contiguous(memory_format=torch.channels_last_3d), y, dict(cl_weight=None, k=3), (1, 2)
    if name == "c3 hybird ncdhw k1":
        x, y = logits_c3((2,) + BASE[2:], 207)
        return x, y, dict(cl_weight=0.3, k=1), (1, 2)
    if name == "c3 soft classes=(2,)":
        x, y = logits_c3((2,) + BASE[2:], 209)
        return x, y, dict(cl_weight=None, k=2, classes=(2,)), (2,)
    if name == "c3 hybird weighted":
        x, y = logits_c3((2,) + BASE[2:], 211)
        return x, y, dict(cl_weight=0.5, k=3, weight_v=[0.2, 1.0, 3.0], smooth=0.5), (1, 2)
    if name == "c3 hybird tile+1 k0":
        x, y = logits_c3((1,) + TILE_PLUS_ONE[2:], 213)
        return x.contiguous(memory_format=torch.channels_last_3d), y, dict(cl_weight=0.5, k=0), (1, 2)
    if name == "c2 soft line k64":
        x, y = logits_c2((2,) + LINE[2:], 215)
        return x, y, dict(cl_weight=None, k=64), (1,)
    if name == "c2 hybird pair":
        x, y = logits_c2((1,) + PAIR[2:], 217)
        return x, y, dict(cl_weight=0.5, k=3), (1,)
    if name == "c3 hybird upstream 1024":
        x, y = logits_c3((2,) + BASE[2:], 219)
        return x, y, dict(cl_weight=0.5, k=3, upstream=1024.0), (1, 2)
    raise KeyError(name)


# case -> F
LOSS_CASES = {"c2 soft ncdhw": 1.2e-6, "c2 hybird ndhwc u8": 3.0e-7, "c3 soft ndhwc": 3.9e-7, "c3 hybird ncdhw k1": 4.4e-7,
              "c3 soft classes=(2,)": 2.0e-7, "c3 hybird weighted": 8.8e-7, "c3 hybird tile+1 k0": 4.6e-7,
              "c2 soft line k64": 3.3e-7, "c2 hybird pair": 1.9e-6, "c3 hybird upstream 1024": 4.8e-7}
F_BF16 = 5.4e-7


@pytest.mark.parametrize("name", sorted(LOSS_CASES))
def test_losses_value_and_gradient(name):
    x, y, kw, entering = make_case(name)
    assert_well_separated(x, entering, 6e-5 if x.shape[1] == 2 else 1e-5)
    ref_v, ref_g = loss_reference(x, y, **kw)
    v, g = loss_device(x.to(DEV), y.to(DEV), **kw)
    assert_value(v, ref_v, name)
    assert_grad(g, ref_g, name, LOSS_CASES[name])


def test_bf16_logits():
    """The kernels read float32: 16-bit logits are widened first, and the bf16 gradient is the float32 gradient of the
    widened logits rounded once (asserted bit for bit).  That float32 gradient is held to the float64 reference at the
    gate of every other case (F_BF16), so the bf16 gradient is held to the same gate carried through the rounding:
    rounding is monotone, so each element lies between the bf16 roundings of the two ends of its gate.  It differs from
    the rounded reference only where a bf16 rounding boundary falls inside that gate, and then by one bf16 step."""
    x, y = logits_c2_bf16((2,) + SMALL[2:], 221)
    assert x.dtype == torch.bfloat16
    assert_well_separated(x.float(), (1,), 6e-5)
    kw = dict(cl_weight=0.5, k=3)
    ref_v, ref_g = loss_reference(x, y, **kw)
    v, g = loss_device(x.to(DEV), y.to(DEV), **kw)
    assert g.dtype == torch.bfloat16
    assert_value(v, ref_v, "bf16")
    v32, g32 = loss_device(x.float().to(DEV), y.to(DEV), **kw)
    assert torch.equal(v, v32) and torch.equal(g, g32.to(torch.bfloat16))
    assert_grad(g32, ref_g, "bf16 widened", F_BF16)
    tol = GRAD_REL * ref_g.abs() + F_BF16 * float(ref_g.abs().max())
    lo, hi = (ref_g - tol).to(torch.bfloat16).double(), (ref_g + tol).to(torch.bfloat16).double()
    got, want = g.cpu().double(), ref_g.to(torch.bfloat16).double()
    print("bf16: %d of %d elements not the rounded reference, %d could differ" % (
        int((got != want).sum()), got.numel(), int((lo != hi).sum())))
    assert bool(((got >= lo) & (got <= hi)).all())


# ------------------------------------------------------------------------------------------------ bit equalities
def test_cl_weight_zero_is_hybird_loss():
    x, y = logits_c3((2,) + BASE[2:], 231)
    for layout in ("ncdhw", "ndhwc"):
        xx = (x if layout == "ncdhw" else x.contiguous(memory_format=torch.channels_last_3d)).to(DEV)
        a = xx.detach().requires_grad_(True)
        va = L.HybirdClDiceLoss(cl_weight=0.0, weight_v=[1.0, 2.0, 3.0])(a, y.to(DEV))
        va.backward()
        b = xx.detach().requires_grad_(True)
        vb = L.HybirdLoss(weight_v=[1.0, 2.0, 3.0])(b, y.to(DEV))
        vb.backward()
        assert torch.equal(va, vb) and torch.equal(a.grad, b.grad), layout


def test_cl_weight_one_is_soft_cldice():
    x, y = logits_c3((2,) + BASE[2:], 233)
    va, ga = loss_device(x.to(DEV), y.to(DEV), 1.0, 3, weight_v=[1.0, 2.0, 3.0])
    vb, gb = loss_device(x.to(DEV), y.to(DEV), None, 3, weight_v=[1.0, 2.0, 3.0])
    assert torch.equal(va, vb) and torch.equal(ga, gb)


def test_same_input_same_bits():
    x, y = logits_c3((2,) + BASE[2:], 241)
    big = torch.randn((2, 3, 19, 21, 70), generator=torch.Generator().manual_seed(5))
    ybig = torch.randint(0, 3, (2, 19, 21, 70), generator=torch.Generator().manual_seed(6))
    for xx, yy in ((x, y), (big, ybig)):
        for cl_weight in (None, 0.5):
            v1, g1 = loss_device(xx.to(DEV), yy.to(DEV), cl_weight, 3)
            v2, g2 = loss_device(xx.to(DEV), yy.to(DEV), cl_weight, 3)
            assert torch.equal(v1, v2) and torch.equal(g1, g2)


@pytest.mark.parametrize("cl_weight", [None, 0.5])
def test_label_out_of_range_raises(cl_weight):
    x, y = logits_c3((2,) + BASE[2:], 251)
    y = y.clone()
    y[1, 3, 4, 5] = 3
    L.raise_on_bad_labels(wait=True)
    crit = L.SoftClDiceLoss() if cl_weight is None else L.HybirdClDiceLoss(cl_weight=cl_weight)
    v = crit(x.to(DEV), y.to(DEV))
    with pytest.raises(RuntimeError, match="Class values must be smaller than num_classes."):
        L.raise_on_bad_labels(wait=True)
    assert bool(torch.isnan(v))


def test_argument_errors_on_the_device():
    import _native as N
    with pytest.raises(N.Ru3dError, match="three spatial"):
        L.HybirdClDiceLoss()(torch.zeros(1, 2, 4, 4, device=DEV), torch.zeros(1, 4, 4, dtype=torch.int64, device=DEV))
    with pytest.raises(N.Ru3dError, match="C == 1"):
        L.HybirdClDiceLoss()(torch.zeros(1, 1, 4, 4, 4, device=DEV), torch.zeros(1, 4, 4, 4, dtype=torch.int64, device=DEV))
    with pytest.raises(N.Ru3dError, match="three spatial"):
        L.soft_skeleton(torch.zeros(1, 4, 4, 4, device=DEV))


# ------------------------------------------------------------------------------------------------ captured step
def test_captured_step_equals_eager_loop():
    """Trainer's automatic capture takes HybirdClDiceLoss as it is; three steps leave the eager loop's parameters."""
    import trainer as T

    class Cases(torch.utils.data.Dataset):
        def __init__(self):
            self.items = [{"image": O.synth_image((1, 1, 32, 32, 32), 600 + i)[0],
                           "label": O.phantom_labels(1, (32, 32, 32), 2)[0]} for i in range(3)]

        def __len__(self):
            return len(self.items)

        def __getitem__(self, i):
            return self.items[i]

    def fit(capture):
        torch.manual_seed(5)
        np.random.seed(5)
        ops._drop_counter[0] = 0
        model = network.ResUnet3D(2, 8, 1, 2).to(DEV)
        tr = T.Trainer(model=model, optimizer=optim.Adam(model.parameters(), lr=1e-3), loss=L.HybirdClDiceLoss(),
                       dataset=Cases(), batch_size=1, valid_split=0.0, dataloader_kwargs={"num_workers": 0},
                       metrics={"cldice": L.SoftClDiceLoss(), "both": L.HybirdClDiceLoss()}, progress=False,
                       capture_step=capture)
        tr.fit(num_epochs=1)
        torch.cuda.synchronize()
        return tr, model

    tr_e, m_e = fit(False)
    assert tr_e._graphed is None
    tr_g, m_g = fit(None)
    assert tr_g.graph_stats["replays"] > 0
    assert tr_e.best_result == tr_g.best_result
    for (k, a), (_, b) in zip(m_e.state_dict().items(), m_g.state_dict().items()):
        assert torch.equal(a, b), k
