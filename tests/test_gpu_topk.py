"""The top-k kernels of csrc/topk.hip on a real MI355X: the exact select alone against numpy, and TopKLoss /
HybirdTopKLoss against the float64 definitions, through the loss matrix, saturated logits, built ties, 16-bit logits, bad
labels, the saved ce[], the captured training step and the Trainer's automatic capture.

The select.  Reference: numpy on the same float32 values.  tau is compared bit for bit with np.partition's K-th largest,
count_gt and count_eq with (v > tau).sum() and (v == tau).sum().  The two zeros are one value for numpy's partition, which
hands back whichever of them its own moves left at the position; the kernel's contract is +0, so a zero from numpy is
taken as +0 before the bits are compared, and the kernel's zero must be +0.  sum_gt is held to math.fsum of the selected
values: |err| <= n * 2^-53 * fsum(|selected|), the worst case of n float64 additions (each addition errs by at most
2^-53 of a partial sum, and no partial sum exceeds the sum of the magnitudes).

The losses.  Reference: the definitions ("Top-k loss") in float64 on the float32 logits, written out below, the
gradient by float64 autograd; the scalars enter as the float32 values the kernel is handed.  Tolerances, those of
tests/test_gpu_groups.py / test_gpu_loss_kernels.py for the same reduction structure:
  * value: |err| <= 2e-6 * max(1, |ref|);
  * gradient, element by element: |err| <= 2e-5 * |ref| + 1e-6 * max|ref|.
Selection near the threshold is where float32 and float64 may legitimately disagree: voxels whose float64 ce lies within
1e-5 * max(1, tau) of the float64 tau are left out of the element-wise gradient comparison (never of the value
comparison); every case first asserts that at most 4 voxels are left out and prints how many were.  k = 100 leaves
nothing out.
16-bit logits: the gradient is the float32 gradient of the widened logits rounded once to the logits' type, so the unit
roundoff of that type (2^-8 relative for bfloat16; 2^-11 relative and 2^-25 absolute for float16) is added to the element
bound, as tests/test_gpu_groups.py does.
Run with `-m gpu`."""
import math
import struct

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no HIP device", allow_module_level=True)

import _native as N  # noqa: E402
import _ops as ops  # noqa: E402
import graph  # noqa: E402
import loss as L  # noqa: E402
import network  # noqa: E402
import optim  # noqa: E402
import trainer as T  # noqa: E402
from oracle import unet_oracle as O  # noqa: E402

DEV = torch.device("cuda:0")
VALUE_TOL = 2e-6
GRAD_REL = 2e-5
GRAD_FLOOR = 1e-6
NEAR = 1e-5
MAX_LEFT_OUT = 4
BAD_LABELS = "Class values must be smaller than num_classes."


def f32(x):
    return float(torch.tensor(float(x), dtype=torch.float32))


# ------------------------------------------------------------------------------------------------ the select alone
TRIP = int(N.lib.ru3d_topk_select_trip_elements())
SIZES = [1, 255, 256, 257, 2047, 2049, 65537, TRIP + 5]
INPUTS = ["normal", "equal", "two_values", "last_digit", "zeros_subnormals", "nonnegative"]


def select(values, k):
    """The raw result bytes and (tau bits, count_gt, count_eq, sum_gt) of ru3d_topk_select on a device float32 vector."""
    n = values.numel()
    N.note_device(values.device)
    res = torch.full((32,), 0xAB, dtype=torch.uint8, device=DEV)
    ws = torch.empty(N.lib.ru3d_topk_select_workspace_bytes(n), dtype=torch.uint8, device=DEV)
    N.check(N.lib.ru3d_topk_select(N.ptr(values), n, k, N.ptr(res), N.ptr(ws), ws.numel(), N.stream()), "topk_select")
    raw = bytes(res.cpu().numpy())
    tau_bits, gt, eq, total = struct.unpack("<I4xqqd", raw)
    return raw, (tau_bits, gt, eq, total)


def draw_values(kind, n, k, seed):
    rng = np.random.RandomState(seed)
    if kind == "normal":
        return rng.standard_normal(n).astype(np.float32)
    if kind == "equal":
        return np.full(n, -1.75, dtype=np.float32)
    if kind == "two_values":                           # K falls inside the run of the lower value
        v = np.full(n, 0.25, dtype=np.float32)
        v[rng.permutation(n)[:k // 2]] = 3.5
        return v
    if kind == "last_digit":                           # one key in the upper 22 bits: 1 + r * 2^-23, r < 1024
        return (np.uint32(0x3F800000) | rng.randint(0, 1024, n).astype(np.uint32)).view(np.float32)
    if kind == "zeros_subnormals":
        bits = rng.randint(0, 6, n).astype(np.uint32) | (rng.randint(0, 2, n).astype(np.uint32) << np.uint32(31))
        return bits.view(np.float32)
    v = np.abs(rng.standard_normal(n)).astype(np.float32)
    v[rng.permutation(n)[:n // 3]] = 0.0               # the loss's own case: ce >= 0 with exact zeros
    return v


# every input at every size up to 65537; the size beyond one grid-stride trip on the two drawn inputs
SELECT_CASES = [(n, kind) for n in SIZES for kind in INPUTS if n <= 65537 or kind in ("normal", "nonnegative")]


@pytest.mark.parametrize("n,kind", SELECT_CASES)
def test_select_is_exact(n, kind):
    for k in sorted({kk for kk in (1, 2, n // 10, n - 1, n) if 1 <= kk <= n}):
        v = draw_values(kind, n, k, seed=n % 1000 + k % 7)
        dv = torch.from_numpy(v).to(DEV)
        raw, (tau_bits, gt, eq, total) = select(dv, k)
        raw2, _ = select(dv, k)
        assert raw == raw2, "two runs differ"
        with np.errstate(all="ignore"):
            ref_tau = np.partition(v, n - k)[n - k] + np.float32(0.0)    # a zero of either sign -> +0
            above = v[v > ref_tau].astype(np.float64)
            ref_eq = int((v == ref_tau).sum())
        what = "%s n=%d K=%d" % (kind, n, k)
        assert tau_bits == int(np.float32(ref_tau).view(np.uint32)), "%s: tau %#x, numpy %r" % (what, tau_bits, ref_tau)
        assert gt == above.size and eq == ref_eq, "%s: counts %d %d, numpy %d %d" % (what, gt, eq, above.size, ref_eq)
        ref_sum = math.fsum(above.tolist())
        bound = n * 2.0 ** -53 * math.fsum(np.abs(above).tolist())
        assert abs(total - ref_sum) <= bound, "%s: sum %r, fsum %r, bound %g" % (what, total, ref_sum, bound)
        if kind == "normal" and k == n:
            # the identity the losses use: the mean of the K largest
            mean = (total + (k - gt) * float(ref_tau)) / k
            ref_mean = math.fsum(np.sort(v)[n - k:].astype(np.float64).tolist()) / k
            assert abs(mean - ref_mean) <= bound / k + 1e-15 * abs(ref_mean)


def test_select_ignores_what_lies_beside_the_values():
    """An unaligned start (the 16-byte loads begin at the first boundary) and sentinels on both sides."""
    rng = np.random.RandomState(9)
    host = rng.standard_normal(5000).astype(np.float32)
    host[:3] = 1e30
    host[3 + 4001:] = 1e30
    dv = torch.from_numpy(host).to(DEV)[3:3 + 4001]
    v = host[3:3 + 4001]
    _, (tau_bits, gt, eq, total) = select(dv, 400)
    ref_tau = np.partition(v, 4001 - 400)[4001 - 400]
    assert tau_bits == int(ref_tau.view(np.uint32)) and gt == int((v > ref_tau).sum()) and eq == int((v == ref_tau).sum())
    above = v[v > ref_tau].astype(np.float64)
    assert abs(total - math.fsum(above.tolist())) <= 4001 * 2.0 ** -53 * math.fsum(np.abs(above).tolist())


# ------------------------------------------------------------------------------------------------ the losses: reference
def inputs(c, v, seed):
    g = torch.Generator().manual_seed(seed)
    x = 3 * torch.randn((2, c, v), generator=g)
    y = torch.randint(0, c, (2, v), generator=g)
    return x, y


def on_device(x, y, layout="ncdhw", label_dtype=torch.int64):
    x = x.to(DEV)
    if layout == "ndhwc":
        x = x.movedim(1, -1).contiguous().movedim(-1, 1)           # the same values, the class axis fastest
        assert x.stride(1) == 1 or x.shape[1] == 1
    return x, y.to(label_dtype).to(DEV)


def reference_topk(x, y, k):
    """float64 value and gradient of topk from the definitions, the tie rule included; also the mask of the voxels whose ce
    lies within NEAR of tau (empty when K == M)."""
    z = x.detach().to("cpu", torch.float64).contiguous().requires_grad_(True)
    n, c = z.shape[0], z.shape[1]
    zf = z.reshape(n, c, -1)
    t = y.detach().cpu().long().reshape(n, -1)
    ce = -(torch.log_softmax(zf, 1).gather(1, t[:, None])).reshape(-1)
    m = ce.numel()
    kk = max(1, int(m * k / 100))
    held = ce.detach()
    tau = torch.sort(held, descending=True).values[kk - 1]
    above, tied = held > tau, held == tau
    g, e = int(above.sum()), int(tied.sum())
    s = above.double() + tied.double() * ((kk - g) / e)
    v = (s * ce).sum() / kk
    v.backward()
    near = ((held - tau).abs() <= NEAR * max(1.0, float(tau))).reshape(n, -1)
    if kk == m:
        near = torch.zeros_like(near)
    return float(v.detach()), z.grad.reshape(x.shape), near, (float(tau), g, e, kk)


def reference_dice(x, y, weight_v=None, alpha=0.5, beta=0.5, smooth=1e-7):
    z = x.detach().to("cpu", torch.float64).contiguous().requires_grad_(True)
    n, c = z.shape[0], z.shape[1]
    p = torch.softmax(z.reshape(n, c, -1), 1)
    g = F.one_hot(y.detach().cpu().long().reshape(n, -1), c).movedim(-1, 1).double()
    w = torch.ones(c, dtype=torch.float64) if weight_v is None else torch.tensor([f32(a) for a in weight_v],
                                                                                 dtype=torch.float64)
    w = w / w.abs().sum().clamp_min(1e-12)
    a, b, s = f32(alpha), f32(beta), f32(smooth)
    tp, sp, sg = (p * g).sum((0, 2)), p.sum((0, 2)), g.sum((0, 2))
    v = (w * (1.0 - (tp + s) / (tp + a * (sg - tp) + b * (sp - tp) + s))).sum()
    v.backward()
    return float(v.detach()), z.grad.reshape(x.shape)


def run(crit, x, y, upstream=None):
    """Value and gradient from the HIP kernels; x keeps its strides and its dtype."""
    x = x.detach().requires_grad_(True)
    v = crit(x, y)
    assert v.dim() == 0 and v.is_cuda and v.dtype == torch.float32
    (v if upstream is None else upstream(v)).backward()
    assert x.grad.shape == x.shape and x.grad.dtype == x.dtype and x.grad.stride() == x.stride()
    return v.detach(), x.grad.detach()


def assert_value(got, ref, what):
    got = float(got)
    print("%s: value %.9g, float64 %.9g, error %.3g of the bound" % (what, got, ref,
                                                                    abs(got - ref) / (VALUE_TOL * max(1.0, abs(ref)))))
    assert abs(got - ref) <= VALUE_TOL * max(1.0, abs(ref)), "%s: value %.9g, float64 %.9g" % (what, got, ref)


def assert_grad(got, ref, what, near=None, rel=GRAD_REL, extra_abs=0.0):
    got = got.detach().to("cpu", torch.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), "%s: gradient not finite" % what
    err = (got - ref).abs()
    tol = rel * ref.abs() + GRAD_FLOOR * float(ref.abs().max()) + extra_abs
    compared = torch.ones_like(err, dtype=torch.bool)
    if near is not None:
        left_out = int(near.sum())
        print("%s: %d voxels near the threshold left out of the gradient comparison" % (what, left_out))
        assert left_out <= MAX_LEFT_OUT, "%s: %d voxels near the threshold" % (what, left_out)
        compared = ~near[:, None, :].expand_as(err)
    off = (err > tol) & compared
    worst = float((err / tol.clamp_min(1e-300))[compared].max())
    print("%s: worst compared gradient element %.3g of its bound (max|ref| %.3g)" % (what, worst, float(ref.abs().max())))
    assert not bool(off.any()), "%s: %d gradient elements off, worst %.3g of its bound (max|ref| %.3g)" % (
        what, int(off.sum()), worst, float(ref.abs().max()))


_REFS = {}


def refs(c, v, k, seed):
    """The references of a drawn case, computed once and shared: (x, y, topk value, topk gradient, near mask, stats)."""
    key = (c, v, k, seed)
    if key not in _REFS:
        x, y = inputs(c, v, seed)
        _REFS[key] = (x, y) + reference_topk(x, y, k)
    return _REFS[key]


_DICE = {}


def dice_refs(c, v, seed, **kw):
    key = (c, v, seed, tuple(sorted((a, tuple(b) if isinstance(b, list) else b) for a, b in kw.items())))
    if key not in _DICE:
        x, y = inputs(c, v, seed)
        _DICE[key] = reference_dice(x, y, **kw)
    return _DICE[key]


# ------------------------------------------------------------------------------------------------ the loss matrix
@pytest.mark.parametrize("v", [255, 2047, 2048, 2049, 6000, 32768])
@pytest.mark.parametrize("c", [2, 3, 5, 8])
def test_both_losses_every_class_count_size_layout_and_label_type(c, v):
    seed = 1000 * c + v % 997
    dice_v, dice_g = dice_refs(c, v, seed)
    for k in (0.5, 10, 50, 100):
        x, y, ref_v, ref_g, near, (tau, g, e, kk) = refs(c, v, k, seed)
        for layout in ("ncdhw", "ndhwc"):
            for label_dtype in (torch.int64, torch.uint8):
                dx, dy = on_device(x, y, layout, label_dtype)
                what = "C=%d V=%d k=%g %s %s" % (c, v, k, layout, str(label_dtype)[6:])
                got_v, got_g = run(L.TopKLoss(k=k), dx, dy)
                assert_value(got_v, ref_v, "TopKLoss " + what)
                assert_grad(got_g, ref_g, "TopKLoss " + what, near)
                got_v, got_g = run(L.HybirdTopKLoss(k=k), dx, dy)
                assert_value(got_v, dice_v + ref_v, "HybirdTopKLoss " + what)
                assert_grad(got_g, dice_g + ref_g, "HybirdTopKLoss " + what, near)


def test_k_100_is_the_mean_cross_entropy():
    x, y = inputs(3, 2049, 77)
    dx, dy = on_device(x, y)
    got_v, got_g = run(L.TopKLoss(k=100), dx, dy)
    z = x.double().requires_grad_(True)
    ref = F.cross_entropy(z, y)
    ref.backward()
    assert_value(got_v, float(ref.detach()), "k = 100")
    assert_grad(got_g, z.grad, "k = 100")


def test_weights_alpha_beta_ce_weight_and_upstream():
    c, v, k, seed = 3, 2049, 10, 31
    x, y, ref_v, ref_g, near, _ = refs(c, v, k, seed)
    dx, dy = on_device(x, y, "ndhwc", torch.uint8)
    kw = dict(weight_v=[0.2, 0.0, 3.0], alpha=0.3, beta=0.7, smooth=1e-5)
    dice_v, dice_g = dice_refs(c, v, seed, **kw)
    cw = f32(0.35)
    got_v, got_g = run(L.HybirdTopKLoss(k=k, ce_weight=0.35, **kw), dx, dy)
    assert_value(got_v, dice_v + cw * ref_v, "weighted")
    assert_grad(got_g, dice_g + cw * ref_g, "weighted", near)
    plain_v, plain_g = dice_refs(c, v, seed)
    got_v, got_g = run(L.HybirdTopKLoss(k=k), dx, dy, upstream=lambda t: t * -2.5)
    assert_value(got_v, plain_v + ref_v, "upstream")
    assert_grad(got_g, -2.5 * (plain_g + ref_g), "upstream", near)
    got_v, got_g = run(L.TopKLoss(k=k), dx, dy, upstream=lambda t: t * 0.125)
    assert_grad(got_g, 0.125 * ref_g, "TopKLoss upstream", near)
    # exactly K voxels carry the top-k gradient when nothing ties
    assert int((got_g.abs().sum(1) > 0).sum()) == L.topk_count(2 * v, k)


# ------------------------------------------------------------------------------------------------ ties
@pytest.mark.parametrize("cls", ["TopKLoss", "HybirdTopKLoss"])
def test_saturated_logits_tie_at_zero(cls):
    """|z| = 60: a voxel whose target logit is the only +60 has ce == 0 exactly; about four in five voxels are such, and
    K = M / 2 reaches into them.  The tied voxels are equal in float64 as well (equal logits), so nothing is left out."""
    g = torch.Generator().manual_seed(8)
    c, v = 3, 3000
    y = torch.randint(0, c, (2, v), generator=g)
    x = torch.full((2, c, v), -60.0)
    x.scatter_(1, y[:, None], 60.0)
    wrong = torch.rand((2, v), generator=g) < 0.2
    x = torch.where(wrong[:, None], -x, x)             # a wrong voxel: the target at -60, the two others at +60
    dx, dy = on_device(x, y)
    ref_v, ref_g, _, (tau, gg, e, kk) = reference_topk(x, y, 50)
    assert kk > gg and e > 1000 and tau < 1e-40         # the threshold sits among the saturated voxels
    crit = L.TopKLoss(k=50) if cls == "TopKLoss" else L.HybirdTopKLoss(k=50)
    got_v, got_g = run(crit, dx, dy)
    assert bool(torch.isfinite(got_v)) and bool(torch.isfinite(got_g).all())
    if cls == "HybirdTopKLoss":
        dv, dg = reference_dice(x, y)
        ref_v, ref_g = ref_v + dv, ref_g + dg
    assert_value(got_v, ref_v, cls + " saturated")
    assert_grad(got_g, ref_g, cls + " saturated")


def tie_case():
    """float32 (2, 2, 10) logits, 20 voxels, k = 25 -> K = 5: three voxels above the threshold, exactly four tied at it
    (equal logits -> equal ce bits), thirteen below: K - G = 2, a tied voxel gets half weight."""
    margins = [-2.0, -3.0, -4.0] + [0.5] * 4 + [1.0 + 0.125 * i for i in range(13)]
    order = torch.randperm(20, generator=torch.Generator().manual_seed(3))
    m = torch.tensor(margins)[order]
    flat_y = (torch.arange(20) % 2)[order]
    xv = torch.zeros(20, 2)
    xv[torch.arange(20), flat_y] = m
    src = order.tolist()
    tied = [i for i, s in enumerate(src) if 3 <= s < 7]
    above = [i for i, s in enumerate(src) if s < 3]
    below = [i for i, s in enumerate(src) if s >= 7]
    return xv.reshape(2, 10, 2).movedim(-1, 1).contiguous(), flat_y.reshape(2, 10), above, tied, below


def test_built_ties_get_half_weight_bit_equal_between_runs():
    x, y, above, tied, below = tie_case()
    dx, dy = on_device(x, y)
    v1, g1 = run(L.TopKLoss(k=25), dx, dy)
    v2, g2 = run(L.TopKLoss(k=25), dx, dy)
    assert torch.equal(v1, v2) and torch.equal(g1, g2)
    ref_v, ref_g, _, (tau, g, e, kk) = reference_topk(x, y, 25)
    assert (g, e, kk) == (3, 4, 5)
    assert_value(v1, ref_v, "built ties")
    assert_grad(g1, ref_g, "built ties")
    ce = F.cross_entropy(x.double(), y, reduction="none").reshape(-1)
    assert abs(float(v1) - float(torch.topk(ce, 5).values.mean())) <= VALUE_TOL
    gv = g1.cpu().movedim(1, -1).reshape(20, 2)
    p = torch.softmax(x, 1).movedim(1, -1).reshape(20, 2)
    full = (p - F.one_hot(y.reshape(-1), 2).float()) / 5
    assert torch.allclose(gv[tied], 0.5 * full[tied], rtol=1e-5, atol=0)
    assert torch.allclose(gv[above], full[above], rtol=1e-5, atol=0)
    assert bool((gv[below] == 0).all())
    labels = y.reshape(-1).tolist()
    for i in tied:                                     # tied voxels with one label: equal logits, equal gradient bits
        for j in tied:
            assert labels[i] != labels[j] or torch.equal(gv[i], gv[j])
    assert sorted(labels[i] for i in tied) == [0, 0, 1, 1]


def test_same_input_same_bits():
    x, y = inputs(5, 32768, 42)
    dx, dy = on_device(x, y, "ndhwc", torch.uint8)
    a = run(L.HybirdTopKLoss(), dx, dy)
    b = run(L.HybirdTopKLoss(), dx, dy)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ------------------------------------------------------------------------------------------------ 16-bit logits
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_sixteen_bit_logits(dtype):
    x, y = inputs(3, 2049, 23)
    x = x.to(dtype)
    dx, dy = on_device(x, y)
    v, gx = run(L.HybirdTopKLoss(), dx, dy)
    assert gx.dtype == dtype
    ref_v, ref_g, near, _ = reference_topk(x.float(), y, 10)
    dice_v, dice_g = reference_dice(x.float(), y)
    assert_value(v, dice_v + ref_v, "%s logits" % dtype)
    half_ulp, floor = (2.0 ** -8, 0.0) if dtype == torch.bfloat16 else (2.0 ** -11, 2.0 ** -25)
    assert_grad(gx, dice_g + ref_g, "%s logits" % dtype, near, rel=GRAD_REL + half_ulp, extra_abs=floor)


# ------------------------------------------------------------------------------------------------ bad labels
@pytest.mark.parametrize("cls", ["TopKLoss", "HybirdTopKLoss"])
def test_a_label_out_of_range(cls):
    L.raise_on_bad_labels(wait=True)
    x, y = inputs(3, 600, 41)
    dx, dy = on_device(x, y)
    dy[1, 77] = 3
    crit = getattr(L, cls)()
    v = crit(dx, dy)
    with pytest.raises(RuntimeError, match=BAD_LABELS):
        L.raise_on_bad_labels(wait=True)
    assert bool(torch.isnan(v))
    dy[1, 77] = 2
    v = crit(dx, dy)
    L.raise_on_bad_labels(wait=True)
    assert bool(torch.isfinite(v))
    dy[1, 77] = 3
    crit.check_labels = True                           # the blocking check: raises before the launch
    with pytest.raises(RuntimeError, match=BAD_LABELS):
        crit(dx, dy)
    L.raise_on_bad_labels(wait=True)


def test_state_block():
    """The state begins like every fused loss's (the bad-label count at the shared offset) and continues with tau, G, E, K
    and the two backward weights; ce of a voxel with a label out of range is 0."""
    x, y = inputs(3, 2049, 51)
    dx, dy = on_device(x, y)
    dy[0, 5] = 7
    n, c, v = 2, 3, 2049
    kk = L.topk_count(n * v, 10)
    N.note_device(DEV)
    # what production hands over is torch.empty: the forward initialises the state block and its scratch itself
    state = torch.empty(N.lib.ru3d_topk_loss_state_bytes(), dtype=torch.uint8, device=DEV).fill_(0xFF)
    out = torch.empty((), device=DEV)
    ce = torch.full((n * v,), -1.0, device=DEV)
    ws = torch.empty(N.lib.ru3d_topk_loss_workspace_bytes(n, v, c), dtype=torch.uint8, device=DEV).fill_(0xFF)
    N.check(N.lib.ru3d_topk_loss_fwd(N.ptr(dx), c * v, v, 1, N.ptr(dy), N.LABEL_I64, n, v, c, kk, 1, None, 0.5, 0.5, 1e-7,
                                     0.5, N.ptr(ce), N.ptr(state), N.ptr(out), N.ptr(ws), ws.numel(), N.stream()), "fwd")
    off = N.lib.ru3d_loss_state_bad_labels_offset()
    assert int(state[off:off + 4].view(torch.int32)) == 1 and bool(torch.isnan(out))
    assert float(ce[5]) == 0.0
    ref = F.cross_entropy(x.double(), y, reduction="none").reshape(-1)
    keep = torch.ones(n * v, dtype=torch.bool)
    keep[5] = False
    assert float((ce.cpu().double() - ref)[keep].abs().max()) <= 2e-6 * float(ref.max())
    tail = state[off + 4:].cpu()                       # the count is the last field of the shared head
    tau = float(tail[:4].view(torch.float32))
    g, e, k_state = tail[8:32].view(torch.int64).tolist()
    w_gt, w_eq = tail[32:40].view(torch.float32).tolist()
    held = ce.cpu()
    assert tau == float(torch.sort(held, descending=True).values[kk - 1])
    assert g == int((held > tau).sum()) and e == int((held == tau).sum()) and k_state == kk
    assert w_gt == f32(0.5 / kk) and w_eq == f32(0.5 * (kk - g) / (e * kk))


# ------------------------------------------------------------------------------------------------ the saved ce[]
def test_saved_ce_survives_another_loss_call():
    """Two forwards, then the two backwards in reverse order: both equal their single runs, bit for bit."""
    xa, ya = on_device(*inputs(3, 6000, 61))
    xb, yb = on_device(*inputs(3, 6000, 62))
    crit = L.HybirdTopKLoss(k=10)
    va, ga = run(crit, xa, ya)
    vb, gb = run(crit, xb, yb)
    assert not torch.equal(ga, gb)
    ra, rb = xa.detach().requires_grad_(True), xb.detach().requires_grad_(True)
    la = crit(ra, ya)
    lb = crit(rb, yb)
    L.HybirdLoss()(xa, ya)                             # another tenant of the shared workspace in between
    lb.backward()
    la.backward()
    assert torch.equal(la.detach(), va) and torch.equal(lb.detach(), vb)
    assert torch.equal(ra.grad, ga) and torch.equal(rb.grad, gb)


# ------------------------------------------------------------------------------------------------ captured step
def _batches(n):
    return [(O.synth_image((1, 1, 32, 32, 32), 700 + i).to(DEV), O.phantom_labels(1, (32, 32, 32), 3).to(DEV))
            for i in range(n)]


def _setup():
    torch.manual_seed(5)
    np.random.seed(5)
    ops._drop_counter[0] = 0
    model = network.ResUnet3D(2, 8, 1, 3).to(DEV)
    model.train()
    return model, optim.Adam(model.parameters(), lr=1e-3), L.HybirdTopKLoss(k=10)


def test_captured_step_equals_the_eager_loop():
    """Three steps through GraphedTrainStep leave the eager loop's losses and parameters, bit for bit."""
    batches = _batches(3)
    assert int(batches[0][1].max()) == 2

    def run_steps(graphed):
        model, opt, crit = _setup()
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
            assert step.eager_steps == 1 and step.replays == 2
            L.raise_on_bad_labels(wait=True)
            step.release()
        return losses, params

    l_e, p_e = run_steps(False)
    l_g, p_g = run_steps(True)
    assert l_e == l_g, (l_e, l_g)
    assert all(np.isfinite(l_e)) and l_e[0] != l_e[1]
    bad = [k for k in p_e if not torch.equal(p_e[k], p_g[k])]
    assert not bad, bad


def test_trainer_captures_the_topk_loss_automatically():
    class Cases(torch.utils.data.Dataset):
        def __init__(self):
            self.items = [{"image": O.synth_image((1, 1, 32, 32, 32), 700 + i)[0],
                           "label": O.phantom_labels(1, (32, 32, 32), 3)[0]} for i in range(3)]

        def __len__(self):
            return len(self.items)

        def __getitem__(self, i):
            return self.items[i]

    torch.manual_seed(5)
    np.random.seed(5)
    ops._drop_counter[0] = 0
    model = network.ResUnet3D(2, 8, 1, 3).to(DEV)
    tr = T.Trainer(model=model, optimizer=optim.Adam(model.parameters(), lr=1e-3), loss=L.HybirdTopKLoss(k=10),
                   dataset=Cases(), batch_size=1, valid_split=0.0, dataloader_kwargs={"num_workers": 0},
                   metrics={"dice": L.Dice()}, progress=False, capture_step=None)
    tr.fit(num_epochs=1)
    torch.cuda.synchronize()
    assert tr.graph_stats["replays"] > 0
    tr._release_graph()
