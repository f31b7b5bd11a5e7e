"""The label-group kernels of csrc/groups.hip on a real MI355X: the fused sigmoid + binary focal + Tversky loss (forward
sums, finalize, backward) for every group count, kind and layout, the branches of the focal exponent, voxel counts around
the 256-thread / 2048-voxel layout of the reduction, saturated logits, label types, weights, the ignore label, bad labels,
16-bit logits, the bf16 output of the C ABI, reproducibility and the captured training step; the sliding-window
accumulate and the decoding merge alone and through predict_per_patch; evaluate_groups_case on HIP operands.

Reference of the losses: the definitions ("Label groups") in float64 on the float32 logits, written out below,
the gradient by float64 autograd; 1 - p is taken as sigmoid(-z) there, so that the reference itself does not cancel at
saturated logits.  The scalars (gamma, alpha, beta, smooth, weights) enter as the float32 values the kernel is handed.

Tolerances of the losses, those of tests/test_gpu_loss_kernels.py for the same reduction structure (float32 within a
thread and a wave, float64 from the block row on):
  * value: |err| <= 2e-6 * max(1, |ref|);
  * gradient, element by element: |err| <= 2e-5 * |ref| + 1e-6 * max|ref|.
The host float32 evaluation of these formulas (the torch twin of loss.py on .float() inputs, which is not the kernel) was
held against the same float64 reference on every case of this file's loss matrix, exponent, count, variant and ignore
tests: it stays inside both bounds everywhere (worst value error 0.049 of its bound, worst gradient element 0.34 of its
bound), so neither bound is widened.
16-bit logits: the gradient is the float32 gradient of the widened logits rounded once to the logits' type, so the unit
roundoff of that type (2^-8 relative for bfloat16 with its 8 significant bits; 2^-11 relative for float16 with its 11,
and 2^-25 absolute, half its subnormal spacing) is added to the element bound.
Predict kernels: cnt is a sum of float32 weights in launch order and must be equal; acc is held to 1e-6 of the same
float32 arithmetic on the host (the sigmoid is the one rounding that may differ, 1e-7 per window, at most 4 windows on
a voxel).
Run with `-m gpu`."""
import ctypes

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
import inference as I  # noqa: E402
import loss as L  # noqa: E402
import network  # noqa: E402
import optim  # noqa: E402
import trainer as T  # noqa: E402
import transform as TR  # noqa: E402
from oracle import unet_oracle as O  # noqa: E402

DEV = torch.device("cuda:0")
KINDS = ["GroupHybirdLoss", "GroupDiceLoss", "GroupFocalLoss", "GroupDice"]
NESTED = ((1, 2), (2,))
VALUE_TOL = 2e-6
GRAD_REL = 2e-5
GRAD_FLOOR = 1e-6
BAD_LABELS = "Class values must be smaller than num_classes."


def f32(x):
    return float(torch.tensor(float(x), dtype=torch.float32))


def draw_groups(k, t, seed):
    """k distinct non-empty groups of label values below t, from a fixed seed."""
    rng = np.random.RandomState(seed)
    seen, out = set(), []
    while len(out) < k:
        g = tuple(sorted(rng.choice(t, size=rng.randint(1, 4), replace=False).tolist()))
        if g not in seen:
            seen.add(g)
            out.append(g)
    return tuple(out)


def make(kind, groups, num_labels=None, ignore_label=None, gamma=2, weight_v=None, alpha=0.5, beta=0.5, smooth=1e-7):
    common = dict(num_labels=num_labels, ignore_label=ignore_label, weight_v=weight_v)
    if kind == "GroupHybirdLoss":
        return L.GroupHybirdLoss(groups, gamma=gamma, alpha=alpha, beta=beta, smooth=smooth, **common)
    if kind == "GroupFocalLoss":
        return L.GroupFocalLoss(groups, gamma=gamma, **common)
    return getattr(L, kind)(groups, alpha=alpha, beta=beta, smooth=smooth, **common)


def run(kind, x, y, groups, upstream=None, **kw):
    """Value and gradient from the HIP kernels; x keeps its strides and its dtype."""
    x = x.detach().requires_grad_(True)
    v = make(kind, groups, **kw)(x, y)
    assert v.dim() == 0 and v.is_cuda and v.dtype == torch.float32
    (v if upstream is None else upstream(v)).backward()
    assert x.grad.shape == x.shape and x.grad.dtype == x.dtype
    return v.detach(), x.grad.detach()


def reference(kind, x, y, groups, num_labels=None, ignore_label=None, gamma=2, weight_v=None, alpha=0.5, beta=0.5,
              smooth=1e-7):
    """float64 value and gradient on the host, from the definitions."""
    z = x.detach().to("cpu", torch.float64).contiguous().requires_grad_(True)
    n, k = z.shape[0], z.shape[1]
    zf = z.reshape(n, k, -1)
    yf = y.detach().cpu().long().reshape(n, 1, -1)
    c = torch.ones_like(yf, dtype=torch.float64) if ignore_label is None else (yf != ignore_label).double()
    g = torch.zeros(zf.shape, dtype=torch.float64)
    for q, group in enumerate(groups):
        for t in group:
            g[:, q:q + 1] += (yf == t).double()
    g = g * c
    p, om = torch.sigmoid(zf), torch.sigmoid(-zf)
    w = torch.ones(k, dtype=torch.float64) if weight_v is None else torch.tensor([f32(a) for a in weight_v],
                                                                                 dtype=torch.float64)
    w = w / w.abs().sum().clamp_min(1e-12)
    a, b, s, gm = f32(alpha), f32(beta), f32(smooth), f32(gamma)
    tp, sp, sg = (p * g).sum((0, 2)), (p * c).sum((0, 2)), g.sum((0, 2))
    dice = (tp + s) / (tp + a * (sg - tp) + b * (sp - tp) + s)
    pos, neg = F.softplus(-zf), F.softplus(zf)                    # -log p, -log(1 - p)
    if gm != 0.0:
        pos, neg = om ** gm * pos, p ** gm * neg
    focal = (g * pos + (c - g) * neg).sum((0, 2)) / max(float(c.sum()), 1.0)
    v = (w * {"GroupHybirdLoss": 1.0 - dice + focal, "GroupDiceLoss": 1.0 - dice, "GroupFocalLoss": focal,
              "GroupDice": dice}[kind]).sum()
    v.backward()
    return float(v.detach()), z.grad


def assert_value(got, ref, what):
    got = float(got)
    print("%s: value %.9g, float64 %.9g, error %.3g of the bound" % (what, got, ref,
                                                                    abs(got - ref) / (VALUE_TOL * max(1.0, abs(ref)))))
    assert abs(got - ref) <= VALUE_TOL * max(1.0, abs(ref)), "%s: value %.9g, float64 %.9g" % (what, got, ref)


def assert_grad(got, ref, what, rel=GRAD_REL, extra_abs=0.0):
    got = got.detach().to("cpu", torch.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), "%s: gradient not finite" % what
    err = (got - ref).abs()
    tol = rel * ref.abs() + GRAD_FLOOR * float(ref.abs().max()) + extra_abs
    worst = float((err / tol.clamp_min(1e-300)).max())
    print("%s: worst gradient element %.3g of its bound (max|ref| %.3g)" % (what, worst, float(ref.abs().max())))
    assert not bool((err > tol).any()), "%s: %d gradient elements off, worst %.3g of its bound (max|ref| %.3g)" % (
        what, int((err > tol).sum()), worst, float(ref.abs().max()))


def check(kind, x, y, groups, what, upstream=None, scale=1.0, **kw):
    v, gx = run(kind, x, y, groups, upstream=upstream, **kw)
    ref_v, ref_g = reference(kind, x.float(), y, groups, **kw)
    assert_value(v, ref_v, what)
    assert_grad(gx, ref_g * scale, what)
    return v, gx


def logits_and_labels(shape, k, t, seed, layout="ncdhw", label_dtype=torch.int64):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((shape[0], k) + tuple(shape[1:]), generator=g) * 2.5
    y = torch.randint(0, t, tuple(shape), generator=g).to(label_dtype)
    x = x.to(DEV)
    if layout == "ndhwc":
        x = x.contiguous(memory_format=torch.channels_last_3d)
    return x, y.to(DEV)


# ------------------------------------------------------------------------------------------------ the loss matrix
@pytest.mark.parametrize("layout", ["ncdhw", "ndhwc"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k", range(1, 9))
def test_every_group_count_kind_and_layout(k, kind, layout):
    groups = draw_groups(k, 6, seed=k)
    x, y = logits_and_labels((2, 5, 6, 7), k, 6, seed=100 + k, layout=layout)
    v, gx = check(kind, x, y, groups, "%s k=%d %s" % (kind, k, layout), num_labels=6)
    assert gx.stride() == x.stride()
    if layout == "ndhwc" and k > 1:
        assert x.stride(1) == 1


@pytest.mark.parametrize("kind", ["GroupHybirdLoss", "GroupFocalLoss"])
@pytest.mark.parametrize("gamma", [0, 1, 2, 1.5])
def test_focal_exponent_branches(kind, gamma):
    groups = ((1, 2), (2,), (0, 3))
    x, y = logits_and_labels((2, 5, 6, 7), 3, 4, seed=7)
    check(kind, x, y, groups, "%s gamma=%s" % (kind, gamma), gamma=gamma)


def test_focal_gamma_zero_is_binary_cross_entropy():
    groups = ((1, 2), (2,), (0, 3))
    x, y = logits_and_labels((2, 5, 6, 7), 3, 4, seed=8)
    multi_hot = torch.from_numpy(TR.labels_to_groups(y.cpu().numpy(), groups)).movedim(0, 1).double()
    want = torch.stack([F.binary_cross_entropy_with_logits(x.cpu().double()[:, c], multi_hot[:, c], reduction='mean')
                        for c in range(3)]).mean()
    assert_value(L.GroupFocalLoss(groups, gamma=0)(x, y), float(want), "gamma 0 against BCE-with-logits")


@pytest.mark.parametrize("count", [1, 255, 256, 257, 2047, 2048, 2049, 2048 * 2048 + 3])
def test_voxel_counts_around_the_reduction_layout(count):
    """One thread, one block short of full / full / one beyond, eight voxels a thread short of / at / beyond the second
    block, and a count beyond 2048 blocks x 2048 voxels, where a thread's grid-stride loop takes a ninth turn."""
    x, y = logits_and_labels((1, count), 2, 3, seed=count % 1000)
    for kind in ("GroupHybirdLoss", "GroupDice"):
        check(kind, x, y, NESTED, "%s N*V=%d" % (kind, count))


def test_two_samples_split_the_count():
    x, y = logits_and_labels((2, 1024), 2, 3, seed=11)          # N * V = 2048 over two samples: i / v and i % v both move
    check("GroupHybirdLoss", x, y, NESTED, "two samples of 1024")
    x, y = logits_and_labels((3, 683), 2, 3, seed=12)           # 2049
    check("GroupHybirdLoss", x, y, NESTED, "three samples of 683")


# ------------------------------------------------------------------------------------------------ saturated logits
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("gamma", [0, 2])
def test_saturated_logits(kind, gamma):
    """+-40 against targets of both values: sigmoid(40) == 1 in float32, so log(1 - p) of the rounded p is -inf; the
    kernel takes both logarithms from the logit."""
    assert float(torch.sigmoid(torch.tensor(40.0))) == 1.0
    x = torch.empty(1, 2, 4, 4, 4)
    x[:, 0] = 40.0
    x[:, 1] = -40.0
    x[0, :, 1::2] *= -1.0
    y = torch.zeros(1, 4, 4, 4, dtype=torch.int64)
    y[0, :, 1::2] = 2                                             # both channels on
    y[0, :, :, 2:] = 1                                            # channel 0 on, channel 1 off
    x, y = x.to(DEV), y.to(DEV)
    v, gx = run(kind, x, y, NESTED, gamma=gamma)
    ref_v, ref_g = reference(kind, x, y, NESTED, gamma=gamma)
    assert bool(torch.isfinite(v)) and bool(torch.isfinite(gx).all())
    assert_value(v, ref_v, "%s gamma=%s saturated" % (kind, gamma))
    if kind in ("GroupHybirdLoss", "GroupFocalLoss"):
        assert ref_v > 5.0                                        # the wrong half of the voxels costs 40 each


# ------------------------------------------------------------------------------------------------ operand variants
@pytest.mark.parametrize("label_dtype", [torch.int64, torch.uint8])
def test_label_dtypes(label_dtype):
    x, y = logits_and_labels((2, 5, 6, 7), 2, 3, seed=21, label_dtype=label_dtype)
    check("GroupHybirdLoss", x, y, NESTED, "labels %s" % label_dtype)


@pytest.mark.parametrize("kind", KINDS)
def test_weights_alpha_beta_and_upstream(kind):
    groups = ((1, 2), (2,), (3,))
    x, y = logits_and_labels((2, 5, 6, 7), 3, 4, seed=22)
    check(kind, x, y, groups, "%s weighted" % kind, weight_v=[0.2, 0.0, 3.0], alpha=0.3, beta=0.7, smooth=1e-5)
    check(kind, x, y, groups, "%s upstream" % kind, upstream=lambda v: v * -2.5, scale=-2.5, weight_v=[1.0, 2.0, 0.5])
    # a zero weight silences its channel entirely
    _, gx = run(kind, x, y, groups, weight_v=[0.2, 0.0, 3.0])
    assert bool((gx[:, 1] == 0).all()) and bool((gx[:, 0] != 0).any())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_sixteen_bit_logits(dtype):
    x, y = logits_and_labels((2, 5, 6, 7), 2, 3, seed=23)
    x = x.to(dtype)
    v, gx = run("GroupHybirdLoss", x, y, NESTED)
    assert gx.dtype == dtype and gx.stride() == x.stride()
    ref_v, ref_g = reference("GroupHybirdLoss", x.float(), y, NESTED)
    assert_value(v, ref_v, "%s logits" % dtype)
    half_ulp, floor = (2.0 ** -8, 0.0) if dtype == torch.bfloat16 else (2.0 ** -11, 2.0 ** -25)
    assert_grad(gx, ref_g, "%s logits" % dtype, rel=GRAD_REL + half_ulp, extra_abs=floor)


def c_abi(x, y, groups, kind=N.LOSS_HYBIRD, gamma=2.0, dz_dtypes=(N.F32,), ignore=None):
    """The entry points called directly: loss value, the gradients in the asked dtypes, the state block."""
    n, k = x.shape[0], x.shape[1]
    v = x[0, 0].numel()
    table = L.group_table(groups)
    st = L._flat_strides(x)
    N.note_device(x.device)
    # what production hands over is torch.empty: the forward initialises the state block and its scratch itself
    state = torch.empty(N.lib.ru3d_group_loss_state_bytes(), dtype=torch.uint8, device=DEV).fill_(0xFF)
    out = torch.empty((), device=DEV)
    ws = torch.empty(N.lib.ru3d_group_loss_workspace_bytes(n, v, k), dtype=torch.uint8, device=DEV).fill_(0xFF)
    code = N.LABEL_I64 if y.dtype == torch.int64 else N.LABEL_U8
    group = (k, table, len(table), 0 if ignore is None else 1, 0 if ignore is None else ignore)
    N.check(N.lib.ru3d_group_loss_fwd(N.ptr(x), st[0], st[1], st[2], N.ptr(y), code, n, v, *group, kind, gamma, None,
                                      0.5, 0.5, 1e-7, N.ptr(state), N.ptr(out), N.ptr(ws), ws.numel(), N.stream()),
            "group_loss_fwd")
    grads = []
    for dt in dz_dtypes:
        dz = torch.empty_like(x, dtype=torch.float32 if dt == N.F32 else torch.bfloat16)
        assert dz.stride() == x.stride()
        N.check(N.lib.ru3d_group_loss_bwd(N.ptr(x), st[0], st[1], st[2], N.ptr(y), code, n, v, *group, gamma,
                                          N.ptr(state), None, N.ptr(dz), dt, N.stream()), "group_loss_bwd")
        grads.append(dz)
    return out, grads, state


def test_c_abi_bf16_dlogits_is_the_fp32_one_rounded_once():
    x, y = logits_and_labels((2, 5, 6, 7), 3, 4, seed=24, layout="ndhwc")
    groups = ((1, 2), (2,), (0, 3))
    out, (g32, g16), state = c_abi(x, y, groups, dz_dtypes=(N.F32, N.BF16))
    ref_v, ref_g = reference("GroupHybirdLoss", x, y, groups)
    assert_value(out, ref_v, "C ABI value")
    assert_grad(g32, ref_g, "C ABI f32 dlogits")                  # a NULL grad_out is an upstream gradient of 1
    assert g16.dtype == torch.bfloat16
    err = (g16.float() - g32).abs()
    assert bool((err <= 2.0 ** -8 * g32.abs()).all())
    assert torch.equal(g16, g32.to(torch.bfloat16))
    # the state block: the counted voxels behind the shared coefficients, no bad labels
    off = N.lib.ru3d_loss_state_bad_labels_offset()
    assert int(state[off:off + 4].view(torch.int32)) == 0
    assert float(state[-8:].view(torch.float64)) == 2 * 5 * 6 * 7


# ------------------------------------------------------------------------------------------------ ignore label
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("ignore,label_dtype", [(255, torch.uint8), (-1, torch.int64)])
def test_ignore_label_equals_the_host_twin(kind, ignore, label_dtype):
    x, y = logits_and_labels((2, 5, 6, 7), 2, 3, seed=31)
    drop = (torch.rand(y.shape, generator=torch.Generator().manual_seed(32)) < 0.3).to(DEV)
    yi = torch.where(drop, torch.full_like(y, ignore), y).to(label_dtype)
    v, gx = check(kind, x, yi, NESTED, "%s ignore %d" % (kind, ignore), ignore_label=ignore)
    assert bool((gx.movedim(1, -1)[drop] == 0).all()) and bool((gx.movedim(1, -1)[~drop] != 0).any())
    xh = x.cpu().double().requires_grad_(True)
    twin = make(kind, NESTED, ignore_label=ignore)(xh, yi.cpu())
    assert_value(v, float(twin.detach()), "%s ignore %d against the twin" % (kind, ignore))
    twin.backward()
    assert_grad(gx, xh.grad, "%s ignore %d against the twin" % (kind, ignore))


@pytest.mark.parametrize("kind", KINDS)
def test_an_all_ignored_batch(kind):
    x, _ = logits_and_labels((2, 5, 6, 7), 2, 3, seed=33)
    y = torch.full((2, 5, 6, 7), 255, dtype=torch.uint8, device=DEV)
    v, gx = run(kind, x, y, NESTED, ignore_label=255)
    assert bool(torch.isfinite(v)) and bool((gx == 0).all())
    assert float(v) == {"GroupHybirdLoss": 0.0, "GroupDiceLoss": 0.0, "GroupFocalLoss": 0.0, "GroupDice": 1.0}[kind]
    L.raise_on_bad_labels(wait=True)


# ------------------------------------------------------------------------------------------------ bad labels, determinism
def test_a_label_equal_to_num_labels_raises_through_the_deferred_check():
    L.raise_on_bad_labels(wait=True)
    x, y = logits_and_labels((2, 5, 6, 7), 2, 3, seed=41)
    y[1, 2, 3, 4] = 3
    v = L.GroupHybirdLoss(NESTED)(x, y)
    with pytest.raises(RuntimeError, match=BAD_LABELS):
        L.raise_on_bad_labels(wait=True)
    assert bool(torch.isnan(v))
    # the ignore label is no bad label; a label beyond it still is
    y[1, 2, 3, 4] = 255
    v = L.GroupHybirdLoss(NESTED, ignore_label=255)(x, y)
    L.raise_on_bad_labels(wait=True)
    assert bool(torch.isfinite(v))
    y[0, 0, 0, 0] = 7
    v = L.GroupHybirdLoss(NESTED, ignore_label=255)(x, y)
    with pytest.raises(RuntimeError, match=BAD_LABELS):
        L.raise_on_bad_labels(wait=True)
    assert bool(torch.isnan(v))
    # check_labels=True checks before the launch
    crit = L.GroupHybirdLoss(NESTED, ignore_label=255)
    crit.check_labels = True
    with pytest.raises(RuntimeError, match=BAD_LABELS):
        crit(x, y)
    with pytest.raises(ValueError, match="channels"):
        L.GroupHybirdLoss(((1,), (2,), (1, 2)))(x, y)


def test_same_input_same_bits():
    x, y = logits_and_labels((2, 40, 41, 42), 3, 4, seed=42, layout="ndhwc")
    groups = ((1, 2), (2,), (0, 3))
    a = run("GroupHybirdLoss", x, y, groups)
    b = run("GroupHybirdLoss", x, y, groups)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ------------------------------------------------------------------------------------------------ captured step
def _batches(n):
    return [(O.synth_image((1, 1, 32, 32, 32), 700 + i).to(DEV), O.phantom_labels(1, (32, 32, 32), 3).to(DEV))
            for i in range(n)]


def _setup():
    torch.manual_seed(5)
    np.random.seed(5)
    ops._drop_counter[0] = 0
    model = network.ResUnet3D(2, 8, 1, 2).to(DEV)
    model.train()
    return model, optim.Adam(model.parameters(), lr=1e-3), L.GroupHybirdLoss(NESTED)


def test_captured_step_equals_the_eager_loop():
    """Three steps through GraphedTrainStep leave the eager loop's losses and parameters, bit for bit; a label out of
    range raises after a replay as it does after an eager step."""
    batches = _batches(4)
    assert int(batches[0][1].max()) == 2

    def run_steps(graphed):
        model, opt, crit = _setup()
        step = graph.GraphedTrainStep(model, crit, opt, warmup=1) if graphed else None
        losses = []
        for x, y in batches[:3]:
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
            x, y = batches[3]
            bad = y.clone()
            bad[0, 3, 4, 5] = 3
            v = step(x, bad)
            assert step.replays == 3
            with pytest.raises(RuntimeError, match=BAD_LABELS):
                L.raise_on_bad_labels(wait=True)
            assert bool(torch.isnan(v))
            step.release()
        return losses, params

    l_e, p_e = run_steps(False)
    l_g, p_g = run_steps(True)
    assert l_e == l_g, (l_e, l_g)
    assert all(np.isfinite(l_e)) and l_e[0] != l_e[1]
    bad = [k for k in p_e if not torch.equal(p_e[k], p_g[k])]
    assert not bad, bad


def test_trainer_captures_the_group_loss_automatically():
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
    model = network.ResUnet3D(2, 8, 1, 2).to(DEV)
    tr = T.Trainer(model=model, optimizer=optim.Adam(model.parameters(), lr=1e-3), loss=L.GroupHybirdLoss(NESTED),
                   dataset=Cases(), batch_size=1, valid_split=0.0, dataloader_kwargs={"num_workers": 0},
                   metrics={"dice": L.GroupDice(NESTED)}, progress=False, capture_step=None)
    tr.fit(num_epochs=1)
    torch.cuda.synchronize()
    assert tr.graph_stats["replays"] > 0
    tr._release_graph()


# ------------------------------------------------------------------------------------------------ predict kernels alone
def _near(q, thr):
    return np.abs(np.nan_to_num(q, nan=10.0) - thr) <= 1e-6


@pytest.mark.parametrize("variant", ["plain", "mirrored_weighted"])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("k", [1, 2, 3, 8])
def test_predict_kernels_against_numpy_on_random_windows(k, dt, variant):
    """ru3d_predict_accumulate_groups / ru3d_predict_merge_groups alone: random logits, four overlapping 8^3 windows of a
    13 x 11 x 17 volume, one of them repeated; against the same float32 arithmetic on the host."""
    # seed 9: the first seed for which the host arithmetic of none of the sixteen cases puts a mean within 1e-6 of a
    # threshold (the closest is 1.1e-5 away; bf16 logits make exact ties common: seeds 3 .. 8 each have one)
    rng = np.random.default_rng(9)
    X, Y, Z = 13, 11, 17
    P = (8, 8, 8)
    weighted = variant == "mirrored_weighted"
    wins = [((0, 0, 0), 0), ((3, 1, 5), 5), ((5, 3, 9), 2), ((3, 1, 5), 5)] if weighted else \
        [((0, 0, 0), 0), ((3, 1, 5), 0), ((5, 3, 9), 0), ((3, 1, 5), 0)]
    tables = [I.gaussian_profile(p, 0.3 + 0.1 * a) for a, p in enumerate(P)]
    dtab = [torch.from_numpy(t).to(DEV) for t in tables]
    w3 = (torch.from_numpy(tables[0])[:, None, None] * torch.from_numpy(tables[1])[None, :, None]) \
        * torch.from_numpy(tables[2])[None, None, :]
    assert w3.dtype == torch.float32
    acc = torch.zeros((X, Y, Z, k), device=DEV)
    cnt = torch.zeros((X, Y, Z), device=DEV)
    racc, rcnt = torch.zeros((X, Y, Z, k)), torch.zeros((X, Y, Z))
    g = [N.ptr(t) for t in dtab] if weighted else [None, None, None]
    for (ox, oy, oz), f in wins:
        z = torch.from_numpy(rng.standard_normal((2,) + P + (k,)).astype(np.float32) * 3).to(dt)
        zd = z.to(DEV).permute(0, 4, 1, 2, 3)
        d = N.desc(zd)
        N.check(N.lib.ru3d_predict_accumulate_groups(ctypes.byref(d), N.dtype_code(dt), 1, f, *g, N.ptr(acc), N.ptr(cnt),
                                                     X, Y, Z, ox, oy, oz, N.stream()), "accumulate_groups")
        p = torch.sigmoid(z[1].float())
        dims = [a for a in range(3) if f >> a & 1]
        p = torch.flip(p, dims) if dims else p
        sl = (slice(ox, ox + P[0]), slice(oy, oy + P[1]), slice(oz, oz + P[2]))
        if weighted:
            racc[sl] += p * w3[..., None]
            rcnt[sl] += w3
        else:
            racc[sl] += p
            rcnt[sl] += 1
    assert torch.equal(cnt.cpu(), rcnt)
    assert float((acc.cpu() - racc).abs().max()) < 1e-6
    assert bool((rcnt == 0).any())                                # part of the volume stays uncovered
    # the probabilities need nothing new; the label map is the decoding rule
    crop, size = (1, 0, 2), (11, 10, 14)
    sl = tuple(slice(c, c + s) for c, s in zip(crop, size))
    prob = torch.empty(size + (k,), device=DEV)
    N.check(N.lib.ru3d_predict_merge(N.ptr(acc), N.ptr(cnt), X, Y, Z, k, *crop, *size, 1, N.ptr(prob), N.stream()))
    with np.errstate(invalid="ignore"):
        rq = (racc / rcnt[..., None])[sl].numpy()
    gq = prob.cpu().numpy()
    assert np.array_equal(np.isnan(gq), np.isnan(rq)) and np.nanmax(np.abs(gq - rq)) < 1e-6
    groups = tuple(tuple(range(q + 1, k + 1)) for q in range(k))  # nested: group q holds q+1 .. k
    labels = tuple(range(11, 11 + k))
    for thr in (0.5, tuple(0.3 + 0.05 * q for q in range(k))):
        thr_k = np.full(k, thr, dtype=np.float32) if np.ndim(thr) == 0 else np.asarray(thr, dtype=np.float32)
        out = torch.full(size, 99, dtype=torch.uint8, device=DEV)
        N.check(N.lib.ru3d_predict_merge_groups(N.ptr(acc), N.ptr(cnt), X, Y, Z, k, (ctypes.c_int32 * k)(*labels),
                                                (ctypes.c_float * k)(*thr_k.tolist()), *crop, *size, N.ptr(out),
                                                N.stream()), "merge_groups")
        got = out.cpu().numpy()
        want = TR.groups_to_labels(gq, groups, group_labels=labels, threshold=thr)
        near_host, near = _near(rq, thr_k).any(axis=-1), _near(gq, thr_k).any(axis=-1)
        assert not near_host.any()                                # the seed: the host arithmetic has no voxel on the edge
        assert near.sum() <= 1
        assert not ((got != want) & ~near).any()
        assert np.array_equal(want[~near], TR.groups_to_labels(rq, groups, group_labels=labels, threshold=thr)[~near])
        assert (got[np.isnan(gq).any(axis=-1)] == 0).all()        # uncovered voxels
        assert set(np.unique(got)) <= {0} | set(labels) and len(np.unique(got)) > 1


def test_predict_kernels_refuse_before_launch():
    z = torch.zeros((1, 8, 8, 8, 2), device=DEV).permute(0, 4, 1, 2, 3)
    d = N.desc(z)
    acc = torch.zeros((8, 8, 8, 2), device=DEV)
    cnt = torch.zeros((8, 8, 8), device=DEV)
    lib = N.lib
    assert lib.ru3d_predict_accumulate_groups(ctypes.byref(d), N.F32, 0, 0, None, None, None, N.ptr(acc), N.ptr(cnt), 8, 8,
                                              8, 1, 0, 0, N.stream()) != 0
    assert b"outside" in lib.ru3d_last_error()
    z9 = torch.zeros((1, 8, 8, 8, 9), device=DEV).permute(0, 4, 1, 2, 3)
    d9 = N.desc(z9)
    a9 = torch.zeros((8, 8, 8, 9), device=DEV)
    assert lib.ru3d_predict_accumulate_groups(ctypes.byref(d9), N.F32, 0, 0, None, None, None, N.ptr(a9), N.ptr(cnt), 8, 8,
                                              8, 0, 0, 0, N.stream()) != 0
    assert b"9 groups" in lib.ru3d_last_error()
    out = torch.zeros((8, 8, 8), dtype=torch.uint8, device=DEV)
    lab, thr = (ctypes.c_int32 * 9)(*range(9)), (ctypes.c_float * 9)(*[0.5] * 9)
    assert lib.ru3d_predict_merge_groups(N.ptr(a9), N.ptr(cnt), 8, 8, 8, 9, lab, thr, 0, 0, 0, 8, 8, 8, N.ptr(out),
                                         N.stream()) != 0
    assert lib.ru3d_predict_merge_groups(N.ptr(acc), N.ptr(cnt), 8, 8, 8, 2, lab, thr, 1, 0, 0, 8, 8, 8, N.ptr(out),
                                         N.stream()) != 0
    torch.cuda.synchronize()
    assert not bool(acc.any()) and not bool(cnt.any()) and not bool(out.any())


# ------------------------------------------------------------------------------------------------ predict_per_patch
def _small_model():
    torch.manual_seed(3)
    model = network.ResUnet3D(1, 4, 1, 2).to(DEV)
    model.eval()
    return model


def test_predict_per_patch_with_groups():
    model = _small_model()
    image = O.synth_image((20, 17, 9, 1), 77).numpy()
    patch = (16, 16, 8)
    kw = dict(groups=NESTED)
    prob = T.predict_per_patch(image, model, 2, patch, 2, False, True, **kw)
    mask = T.predict_per_patch(image, model, 2, patch, 2, False, False, **kw)
    assert prob.dtype == np.float32 and prob.shape == (20, 17, 9, 2)
    assert mask.dtype == np.uint8 and mask.shape == (20, 17, 9)
    covered = ~np.isnan(prob).any(axis=-1)
    assert covered.any() and (prob[covered] > 0).all() and (prob[covered] < 1).all()
    near = _near(prob, 0.5).any(axis=-1)
    assert near.sum() <= 1
    assert np.array_equal(mask[~near], TR.groups_to_labels(prob, NESTED)[~near])
    assert (mask[~covered] == 0).all()
    # sigmoids, not a softmax: the channels do not sum to one
    assert np.abs(prob[covered].sum(axis=-1) - 1).max() > 1e-3
    # explicit labels and thresholds reach the merge
    relabelled = T.predict_per_patch(image, model, 2, patch, 2, False, False, groups=NESTED, group_labels=(5, 9),
                                     threshold=(0.4, 0.6))
    near = (_near(prob[..., 0], 0.4) | _near(prob[..., 1], 0.6))
    want = TR.groups_to_labels(prob, NESTED, group_labels=(5, 9), threshold=(0.4, 0.6))
    assert near.sum() <= 1 and np.array_equal(relabelled[~near], want[~near])
    # patch_batch only decides how many windows share a forward
    for one_hot, first in ((True, prob), (False, mask)):
        again = T.predict_per_patch(image, model, 2, patch, 2, False, one_hot, patch_batch=3, **kw)
        assert np.array_equal(first, again, equal_nan=True)
    with pytest.raises(ValueError, match="groups"):
        T.predict_per_patch(image, model, 3, patch, 2, False, False, **kw)
    with pytest.raises(ValueError):
        T.predict_per_patch(image, model, 2, patch, 2, False, False, groups=((1, 2), (1,)), threshold=float("nan"))


def test_predict_per_patch_blended_with_groups_covers_every_voxel():
    model = _small_model()
    image = O.synth_image((20, 17, 9, 1), 77).numpy()
    kw = dict(groups=NESTED, placement='cover', weighting='gaussian', mirror_axes=(0,))
    prob = T.predict_per_patch(image, model, 2, (16, 16, 8), 2, False, True, **kw)
    mask = T.predict_per_patch(image, model, 2, (16, 16, 8), 2, False, False, **kw)
    assert prob.shape == (20, 17, 9, 2) and not np.isnan(prob).any()
    assert (prob > 0).all() and (prob < 1).all()
    near = _near(prob, 0.5).any(axis=-1)
    assert near.sum() <= 1
    assert np.array_equal(mask[~near], TR.groups_to_labels(prob, NESTED)[~near])
    again = T.predict_per_patch(image, model, 2, (16, 16, 8), 2, False, True, patch_batch=3, **kw)
    assert np.array_equal(prob, again)


def test_predict_per_patch_without_groups_is_the_softmax_route():
    """groups=None: the softmax accumulate and the argmax merge, window by window as before - restated here with the entry
    points called by hand - and not a bit of the result moves."""
    model = _small_model()
    image = O.synth_image((20, 17, 9, 1), 77).numpy()
    patch = (16, 16, 8)
    prob = T.predict_per_patch(image, model, 2, patch, 2, False, True)
    mask = T.predict_per_patch(image, model, 2, patch, 2, False, False)
    full = I.padded_shape(image.shape[:3], patch)
    lo, co = I.pad_offset(image.shape[:3], full), I.crop_offset(image.shape[:3], full)
    vol = torch.zeros((1, 1) + full, device=DEV)
    vol[0, 0, lo[0]:lo[0] + 20, lo[1]:lo[1] + 17, lo[2]:lo[2] + 9] = torch.from_numpy(image[..., 0]).to(DEV)
    acc = torch.zeros(full + (2,), device=DEV)
    cnt = torch.zeros(full, device=DEV)
    origins, _ = I.window_origins(full, patch, 2)
    with torch.no_grad():
        for (ox, oy, oz) in origins:
            x = N.new_act(1, 1, 16, 16, 8, torch.float32, DEV)
            x[0].copy_(vol[0, :, ox:ox + 16, oy:oy + 16, oz:oz + 8])
            logits = N.to_ndhwc(model(x))
            d = N.desc(logits)
            N.check(N.lib.ru3d_predict_accumulate(ctypes.byref(d), N.dtype_code(logits.dtype), 0, N.ptr(acc), N.ptr(cnt),
                                                  full[0], full[1], full[2], ox, oy, oz, N.stream()))
    for one_hot, got in ((1, prob), (0, mask)):
        out = torch.empty((20, 17, 9, 2), device=DEV) if one_hot else torch.empty((20, 17, 9), dtype=torch.uint8, device=DEV)
        N.check(N.lib.ru3d_predict_merge(N.ptr(acc), N.ptr(cnt), full[0], full[1], full[2], 2, co[0], co[1], co[2], 20, 17, 9,
                                         one_hot, N.ptr(out), N.stream()))
        assert np.array_equal(got, out.cpu().numpy(), equal_nan=True)
    covered = ~np.isnan(prob).any(axis=-1)
    assert np.abs(prob[covered].sum(axis=-1) - 1).max() < 1e-6     # a softmax


# ------------------------------------------------------------------------------------------------ evaluate_groups_case
def test_evaluate_groups_case_on_hip_operands_equals_the_numpy_route():
    rng = np.random.RandomState(5)
    label = rng.randint(0, 4, size=(19, 18, 17)).astype(np.uint8)
    pred = np.where(rng.rand(19, 18, 17) < 0.7, label, rng.randint(0, 4, size=(19, 18, 17))).astype(np.uint8)
    groups = ((1, 2), (2,), (3, 1), (5,), (31, 6))
    want = T.evaluate_groups_case({'label': label, 'pred': pred}, groups)
    dl, dp = torch.from_numpy(label).to(DEV), torch.from_numpy(pred).to(DEV)
    assert T.evaluate_groups_case({'label': dl, 'pred': dp}, groups) == want
    assert T.evaluate_groups_case({'label': dl, 'pred': pred}, groups) == want
    assert T.evaluate_groups_case({'label': label, 'pred': dp}, groups) == want
    assert want[3] == 1.0 and want[4] == 1.0 and 0.5 < want[0] < 1.0
