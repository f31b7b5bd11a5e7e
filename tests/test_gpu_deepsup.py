"""Deep supervision on a real MI355X: the multi-level loss kernels of csrc/deepsup.hip against a float64 reference written
here, and the auxiliary heads of network.Unet(deep_supervision=L) on the device routes, in a captured step and under the
Trainer.

Loss reference: softmax in float64 on the float32 logits of every level, the formulas of csrc/loss.hip's header comment
against loss.downsample_labels(target, l), total = sum_l w_l loss_l, the gradients by float64 autograd - as
tests/test_gpu_loss_kernels.py writes its own.  Tolerances are that file's (its header derives them for this arithmetic,
which deepsup.hip runs level by level): value 2e-6 * max(1, |ref|); gradient, element by element,
2e-5 * |ref| + 1e-6 * max|ref|.  Both are applied PER LEVEL - every level's loss to its own reference, every level's
gradient to the maximum of its own reference gradient - so that a coarse level's error cannot hide below level 0's.

Model: every parameter must come out of a deep-supervision backward with a finite, non-zero gradient - except the two
kinds this code base reports as "no gradient" (None) in every net, held by tests/test_gpu_parity.py::test_g1_whole_net_fp32:
a conv bias in front of an InstanceNorm (identically zero) and the skip_conv of a block that does not use it.
Run with `-m gpu`."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no HIP device", allow_module_level=True)

import _ops as ops  # noqa: E402
import graph  # noqa: E402
import loss as L  # noqa: E402
import network  # noqa: E402
import optim  # noqa: E402
import trainer as T  # noqa: E402
from oracle import unet_oracle as O  # noqa: E402

DEV = torch.device("cuda:0")
F = torch.nn.functional
VALUE_TOL = 2e-6
GRAD_REL = 2e-5
GRAD_FLOOR = 1e-6
KINDS = ["HybirdLoss", "DiceLoss", "FocalLoss"]
# full extents -> levels: odd extents and the ceil rule (10 -> 5 -> 3); a cube; 2 * 33 * 9 * 8 = 4752 voxels on level 0: more
# than one 2048-voxel block per sample pair, level 1 is 17 x 5 x 4
EXTENTS = {"20x12x10": ((20, 12, 10), 3), "16x16x16": ((16, 16, 16), 2), "33x9x8": ((33, 9, 8), 2)}


def f32(x):
    return float(torch.tensor(float(x), dtype=torch.float32))


def make_base(kind, gamma=2, weight_v=None, alpha=0.5, beta=0.5, smooth=1e-7):
    if kind == "HybirdLoss":
        return L.HybirdLoss(gamma=gamma, weight_v=weight_v, alpha=alpha, beta=beta, smooth=smooth)
    if kind == "DiceLoss":
        return L.DiceLoss(weight_v=weight_v, alpha=alpha, beta=beta, smooth=smooth)
    return L.FocalLoss(gamma=gamma, weight_v=weight_v)


def level_shapes(full, levels):
    return [tuple(-(-s // (1 << l)) for s in full) for l in range(levels)]


def operands(n, c, full, levels, seed, label_dtype=torch.int64, ndhwc_level=None, spread=2.0):
    g = torch.Generator().manual_seed(seed)
    xs = []
    for l, shape in enumerate(level_shapes(full, levels)):
        if l == ndhwc_level:      # channels last in memory: the layout the network's heads write
            xs.append((spread * torch.randn((n,) + shape + (c,), generator=g)).to(DEV).permute(0, 4, 1, 2, 3))
        else:
            xs.append((spread * torch.randn((n, c) + shape, generator=g)).to(DEV))
    y = torch.randint(0, c, (n,) + tuple(full), generator=g).to(label_dtype)
    assert len(torch.unique(y)) == c      # every class is present at level 0
    return xs, y.to(DEV)


def reference_level(kind, z, y, gamma=2, weight_v=None, alpha=0.5, beta=0.5, smooth=1e-7):
    """One level in float64 on the host (z requires grad); the scalars as the float32 values the kernel is handed."""
    n, c = z.shape[0], z.shape[1]
    zf = z.reshape(n, c, -1)
    yf = y.detach().cpu().long().reshape(n, 1, -1)
    logp = torch.log_softmax(zf, dim=1)
    p = logp.exp()
    g = torch.zeros(zf.shape, dtype=torch.float64).scatter_(1, yf, 1.0)
    w = torch.ones(c, dtype=torch.float64) if weight_v is None else torch.tensor([f32(a) for a in weight_v],
                                                                                 dtype=torch.float64)
    w = w / w.abs().sum().clamp_min(1e-12)
    a, b, s, gm = f32(alpha), f32(beta), f32(smooth), f32(gamma)
    tp, sp, sg = (p * g).sum((0, 2)), p.sum((0, 2)), g.sum((0, 2))
    dice = (tp + s) / (tp + a * (sg - tp) + b * (sp - tp) + s)
    lt, pt = logp.gather(1, yf), p.gather(1, yf)
    per_voxel = -((1.0 - pt) ** gm) * lt if gm != 0.0 else -lt
    focal = torch.zeros(c, dtype=torch.float64).index_add(0, yf.reshape(-1), per_voxel.reshape(-1))
    focal = focal * c / (n * zf.shape[2])
    if kind == "HybirdLoss":
        return (w * (1.0 - dice + focal)).sum()
    if kind == "DiceLoss":
        return (w * (1.0 - dice)).sum()
    return (w * focal).sum()


def reference(kind, xs, y, weights, upstream=None, **kw):
    """(total, [loss_l], [d upstream(total) / d x_l]) in float64."""
    zs = [x.detach().to("cpu", torch.float64).contiguous().requires_grad_(True) for x in xs]
    per = [reference_level(kind, z, L.downsample_labels(y.cpu(), l), **kw) for l, z in enumerate(zs)]
    total = sum(f32(w) * v for w, v in zip(weights, per))
    (total if upstream is None else upstream(total)).backward()
    return float(total.detach()), [float(v.detach()) for v in per], [z.grad for z in zs]


def assert_value(got, ref, what):
    got = float(got)
    assert abs(got - ref) <= VALUE_TOL * max(1.0, abs(ref)), "%s: value %.9g, float64 %.9g" % (what, got, ref)


def assert_grad(got, ref, what):
    got = got.detach().to("cpu", torch.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), "%s: gradient not finite" % what
    err = (got - ref).abs()
    tol = GRAD_REL * ref.abs() + GRAD_FLOOR * float(ref.abs().max())
    bad = err > tol
    assert not bool(bad.any()), "%s: %d gradient elements off, worst %.3g of its bound (max|ref| %.3g)" % (
        what, int(bad.sum()), float((err / tol.clamp_min(1e-300)).max()), float(ref.abs().max()))


def run(crit, xs, y, upstream=None):
    xs = [x.detach().requires_grad_(True) for x in xs]
    v = crit(xs if len(xs) > 1 else xs[0], y)
    assert v.dim() == 0 and v.is_cuda and v.dtype == torch.float32
    (v if upstream is None else upstream(v)).backward()
    for x in xs:
        assert x.grad.shape == x.shape and x.grad.dtype == x.dtype and x.grad.stride() == x.stride()
    return v.detach(), [x.grad.detach() for x in xs]


def check(kind, xs, y, what, weights=None, upstream=None, **kw):
    crit = L.DeepSupervisionLoss(make_base(kind, **kw), weights=weights)
    v, grads = run(crit, xs, y, upstream)
    per = crit.last_level_losses.clone()
    ws = weights if weights is not None else L.deep_supervision_weights(len(xs))
    ref_v, ref_per, ref_g = reference(kind, xs, y, ws, upstream, **kw)
    print("%s: total %.9g (float64 %.9g)" % (what, float(v), ref_v))
    assert_value(v, ref_v, what)
    assert tuple(per.shape) == (len(xs),)
    for l in range(len(xs)):
        err = (grads[l].double().cpu() - ref_g[l]).abs().max()
        print("  level %d: loss %.9g (float64 %.9g), max gradient error %.3g of max|ref| %.3g"
              % (l, float(per[l]), ref_per[l], float(err), float(ref_g[l].abs().max())))
        assert_value(per[l], ref_per[l], "%s level %d" % (what, l))
        assert_grad(grads[l], ref_g[l], "%s level %d" % (what, l))
    return crit


# ------------------------------------------------------------------------------------------------ loss kernels
@pytest.mark.parametrize("extents", list(EXTENTS))
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("c", [2, 3, 4])
def test_every_class_count_kind_and_extent(c, kind, extents):
    full, levels = EXTENTS[extents]
    xs, y = operands(2, c, full, levels, 10 * c + len(kind) + full[0])
    check(kind, xs, y, "%s C=%d %s" % (kind, c, extents))


@pytest.mark.parametrize("label_dtype", [torch.uint8, torch.int64], ids=["uint8", "int64"])
@pytest.mark.parametrize("kind", KINDS)
def test_label_types_class_weights_and_upstream_gradient(kind, label_dtype):
    xs, y = operands(2, 3, (20, 12, 10), 3, 77, label_dtype=label_dtype)
    check(kind, xs, y, "%s weighted" % kind, upstream=lambda v: -2.5 * v, gamma=1.5 if kind != "DiceLoss" else 2,
          weight_v=[0.2, 0.3, 0.5], alpha=0.3, beta=0.7, smooth=1e-5)


@pytest.mark.parametrize("level", [0, 1, 2])
def test_ndhwc_strided_logits_at_one_level(level):
    xs, y = operands(2, 3, (20, 12, 10), 3, 31 + level, ndhwc_level=level)
    assert xs[level].stride(1) == 1 and not xs[level].is_contiguous()
    check("HybirdLoss", xs, y, "NDHWC at level %d" % level, weights=[0.5, 0.3, 0.2])


@pytest.mark.parametrize("extents", ["20x12x10", "33x9x8"])
def test_class_absent_from_the_labels_a_level_picks(extents):
    full, levels = EXTENTS[extents]
    g = torch.Generator().manual_seed(5)
    y = torch.randint(0, 2, (2,) + full, generator=g)
    y[:, 1::2, 1::2, 1::2] = 2      # class 2 lives at odd positions only: no level above 0 ever picks it
    assert 2 in y and all(2 not in L.downsample_labels(y, l) for l in range(1, levels))
    xs = [(2.0 * torch.randn((2, 3) + s, generator=g)).to(DEV) for s in level_shapes(full, levels)]
    for kind in KINDS:
        check(kind, xs, y.to(DEV), "%s class absent above level 0" % kind)


def test_single_tensor_is_the_base_loss():
    xs, y = operands(2, 3, (20, 12, 10), 1, 41)
    base = L.HybirdLoss(weight_v=[0.2, 0.3, 0.5])
    crit = check("HybirdLoss", xs, y, "one level", weight_v=[0.2, 0.3, 0.5])
    # one level runs the same arithmetic (csrc/loss_core.h) over the same partition in the same finalize order, and the
    # level weight 1.0 multiplies exactly: not close to the base loss but equal to it, value and gradient
    plain, gplain = run(base, xs, y)
    # explicit weights are for the list; the single tensor keeps weight 1 (validation with the training criterion)
    cases = (("DeepSupervisionLoss(single tensor)", crit, lambda x: x), ("DeepSupervisionLoss([tensor])", crit, lambda x: [x]),
             ("single tensor, explicit weights", L.DeepSupervisionLoss(base, weights=[0.6, 0.4]), lambda x: x))
    for what, c, wrap in cases:
        x = xs[0].detach().requires_grad_(True)
        v = c(wrap(x), y)
        v.backward()
        assert torch.equal(v.detach(), plain), "%s: value %.9g, HybirdLoss %.9g" % (what, float(v.detach()), float(plain))
        assert torch.equal(x.grad, gplain[0]), "%s: gradient differs from HybirdLoss's" % what


def test_set_weights_takes_effect_in_place():
    xs, y = operands(2, 3, (20, 12, 10), 3, 51)
    crit = L.DeepSupervisionLoss(L.HybirdLoss())
    v1, g1 = run(crit, xs, y)
    where = crit.last_level_losses.data_ptr()
    per1 = crit.last_level_losses.clone()
    new = [0.2, 0.3, 0.5]
    crit.set_weights(new)
    v2, g2 = run(crit, xs, y)
    assert crit.last_level_losses.data_ptr() == where      # the same persistent block
    assert torch.equal(crit.last_level_losses, per1)        # the levels' own losses do not depend on the weights
    ref1, per_ref, gref1 = reference("HybirdLoss", xs, y, L.deep_supervision_weights(3))
    ref2, _, gref2 = reference("HybirdLoss", xs, y, new)
    assert abs(ref1 - ref2) > 1e-3 and float(v1) != float(v2)
    assert_value(v1, ref1, "default weights")
    assert_value(v2, ref2, "after set_weights")
    for l in range(3):
        assert_value(per1[l], per_ref[l], "level %d" % l)
        assert_grad(g1[l], gref1[l], "default weights, level %d" % l)
        assert_grad(g2[l], gref2[l], "after set_weights, level %d" % l)
    # a backward uses the weights of its own forward, whatever is set in between
    xr = [x.detach().requires_grad_(True) for x in xs]
    v = crit(xr, y)
    crit.set_weights([1.0, 0.0, 0.0])
    v.backward()
    for l in range(3):
        assert_grad(xr[l].grad, gref2[l], "weights changed between forward and backward, level %d" % l)


@pytest.mark.parametrize("where", [(0, 0, 0), (1, 1, 1), (19, 11, 9)])
def test_out_of_range_label_raises_wherever_it_sits(where):
    """(1, 1, 1) and (19, 11, 9) are positions no level above 0 picks: the count is taken on level 0."""
    L.raise_on_bad_labels(wait=True)
    xs, y = operands(2, 3, (20, 12, 10), 3, 61)
    y[1][where] = 3
    v = L.DeepSupervisionLoss(L.HybirdLoss())(xs, y)
    with pytest.raises(RuntimeError, match="Class values must be smaller than num_classes"):
        L.raise_on_bad_labels(wait=True)
    assert bool(torch.isnan(v))
    # and a clean call afterwards leaves nothing behind
    y[1][where] = 0
    assert bool(torch.isfinite(L.DeepSupervisionLoss(L.HybirdLoss())(xs, y)))
    L.raise_on_bad_labels(wait=True)


# ------------------------------------------------------------------------------------------------ model
ROUTES = {"fp32": (32, torch.float32), "bf16": (32, torch.bfloat16), "f30_padded_bf16": (30, torch.bfloat16)}
SHAPE = (2, 1, 16, 16, 16)


def _no_dropout(model):
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout3d):
            m.p = 0.0          # train mode without the random masks: the host twin can repeat the pass
    return model


def _model(route, seed=0, cls=network.ResUnet3D):
    features, dtype = ROUTES[route]
    torch.manual_seed(seed)
    model = _no_dropout(cls(2, features, 1, 3, deep_supervision=2)).to(DEV)
    network.set_compute_dtype(model, dtype)
    assert model.net._pad == (route == "f30_padded_bf16")
    return model.train()


def _torch_twin(model):
    """The same model as a float64 CPU torch module - the torch fallback: every block, the stem and the heads run as the
    torch modules they are built from."""
    twin = copy.deepcopy(model).cpu().double()
    for m in twin.modules():
        if hasattr(m, "_native"):
            m._native = False
    twin.net._native_io = False
    twin.net._configure_native()
    return twin


def _batch(seed=700):
    return O.synth_image(SHAPE, seed).to(DEV), O.phantom_labels(SHAPE[0], SHAPE[2:], 3).to(DEV)


def _no_gradient_by_design(model):
    """Keys whose gradient this code base reports as None: conv biases in front of an InstanceNorm (identically zero) and
    the skip_conv of a block with equal widths and stride 1 (constructed, never used)."""
    keys = set()
    for name, m in model.named_modules():
        if isinstance(m, network.ResBlock):
            keys |= {name + ".conv1.bias", name + ".conv2.bias"}
            if not m.uses_skip_conv:
                keys |= {name + ".skip_conv.weight", name + ".skip_conv.bias"}
    return keys


@pytest.mark.parametrize("route", list(ROUTES))
def test_aux_heads_on_the_device_routes(route):
    features, dtype = ROUTES[route]
    model = _model(route)
    net = model.net
    seen = {}
    hook = net.decode_blocks[1].register_forward_hook(lambda m, i, o: seen.__setitem__("dec1", o.detach()))
    x, y = _batch()
    out = model(x)
    hook.remove()
    assert isinstance(out, list) and len(out) == 2
    assert tuple(out[0].shape) == (2, 3, 16, 16, 16) and tuple(out[1].shape) == (2, 3, 8, 8, 8)
    assert all(o.dtype == torch.float32 and o.is_cuda for o in out)
    # the aux logits are the head's conv of decoder level 1's output (un-padded), operands as the storage type holds them
    dec1 = seen["dec1"]
    assert dec1.dtype == dtype and dec1.shape[1] == 64      # 2 * 32 channels, or 2 * 30 padded to 64
    real = 2 * features
    if dec1.shape[1] > real:
        assert float(dec1[:, real:].abs().max()) == 0.0      # pad lanes hold exact zeros
    head = net.ds_heads[0]
    ref = F.conv3d(dec1[:, :real].double().cpu(), head.weight.detach().to(dtype).double().cpu(),
                   head.bias.detach().double().cpu())
    err = float((out[1].detach().double().cpu() - ref).abs().max())
    if dtype == torch.float32:
        # 64 float32 multiply-adds per logit: tests/test_gpu_headstem.py's bound for a float32 accumulation over the channels
        lim = 1e-6 + 2e-5 * float(ref.abs().max())
    else:
        lim = 2.0 ** -8 * float(ref.abs().max())             # one storage rounding (the per-op head tests' EPS)
    print("%s: aux logits max error %.3g (bound %.3g, max|ref| %.3g)" % (route, err, lim, float(ref.abs().max())))
    assert err <= lim, "%s: aux logits off by %.3g > %.3g" % (route, err, lim)
    # eval mode: the single tensor; in parity mode the same numbers as entry 0 (no dropout, InstanceNorm has no running
    # statistics) within tests/test_gpu_parity.py's bound for logits - the inference pass may take other kernels
    model.eval()
    with torch.no_grad():
        single = model(x)
    assert torch.is_tensor(single) and tuple(single.shape) == (2, 3, 16, 16, 16) and single.dtype == torch.float32
    if dtype == torch.float32:
        assert float((single - out[0].detach()).abs().max()) <= 1e-4
    model.train()
    # backward through both heads: every parameter that has a gradient at all gets a finite, non-zero one
    crit = L.DeepSupervisionLoss(L.HybirdLoss())
    crit(out, y).backward()
    absent = _no_gradient_by_design(model)
    for k, p in model.named_parameters():
        if k in absent:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
            continue
        assert p.grad is not None, k
        assert bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0.0, k
    assert {"net.ds_heads.0.weight", "net.ds_heads.0.bias"} <= {k for k, p in model.named_parameters() if p.grad is not None}
    if dtype != torch.float32:
        return
    # fp32 parity mode against the torch fallback.  The bound is the one tests/test_gpu_parity.py holds the whole-net
    # gradients of every configuration but its 32^3 golden one to (test_other_baseline_configs_fp32_vs_float64_oracle): the
    # truth is the float64 run, the yardstick is how far the reference's own float32 arithmetic - the same torch modules in
    # float32 on the CPU - lands from it, and every HIP gradient must be within max(1.5e-2, twice that distance) of its
    # tensor's float64 maximum.  (This net ends in a 4^3 bottleneck: InstanceNorm statistics over 64 voxels.)
    def twin_grads(dtype64):
        twin = _torch_twin(model).train()
        if not dtype64:
            twin = twin.float()
        xin = x.cpu().double() if dtype64 else x.cpu()
        tout = twin(xin)
        assert isinstance(tout, list) and len(tout) == 2
        L.DeepSupervisionLoss(L.HybirdLoss())(tout, y.cpu()).backward()
        return [t.detach() for t in tout], {k: p.grad for k, p in twin.named_parameters() if k not in absent}

    tout, g64 = twin_grads(True)
    _, g32 = twin_grads(False)
    for o, t in zip(out, tout):
        assert float((o.detach().double().cpu() - t).abs().max()) <= 2e-4      # that test's bound for logits
    rel = lambda a, b: float((a.double() - b).abs().max() / b.abs().max().clamp_min(1e-30))      # noqa: E731
    noise = max(rel(g32[k], g64[k]) for k in g64)
    worst = max((rel(p.grad.cpu(), g64[k]), k) for k, p in model.named_parameters() if k in g64)
    print("fp32 gradients vs float64 torch twin: worst %.3g of max (%s); the twin's own float32 run: %.3g" % (worst + (noise,)))
    assert len(g64) >= 20 and "net.ds_heads.0.weight" in g64
    for k, p in model.named_parameters():
        if k in g64:
            err = rel(p.grad.cpu(), g64[k])
            assert err <= max(1.5e-2, 2 * noise), "grad %s: %.3e of max vs float64 (torch float32 noise %.3e)" % (k, err, noise)


def test_checkpointed_and_batchnorm_nets_train_with_aux_heads():
    x, y = _batch(701)
    crit = L.DeepSupervisionLoss(L.HybirdLoss())
    # activation checkpointing: the same bits as without it
    grads = []
    for ckpt in (False, True):
        model = _model("bf16", seed=2)
        network.set_checkpointing(model, ckpt)
        crit(model(x), y).backward()
        grads.append({k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None})
    assert grads[0].keys() == grads[1].keys() and "net.ds_heads.0.weight" in grads[0]
    assert all(torch.equal(grads[0][k], grads[1][k]) for k in grads[0])
    # BatchNorm + attention blocks in training mode
    model = _model("bf16", seed=3, cls=network.ResAttrBNUnet3D)
    out = model(x)
    assert isinstance(out, list) and tuple(out[1].shape) == (2, 3, 8, 8, 8)
    crit(out, y).backward()
    for k in ("net.ds_heads.0.weight", "net.ds_heads.0.bias", "net.conv.weight"):
        g = dict(model.named_parameters())[k].grad
        assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0.0, k


# ------------------------------------------------------------------------------------------------ captured step
def _batches(n):
    out = []
    for i in range(n):
        x = O.synth_image(SHAPE, 900 + i).to(DEV)
        y = O.phantom_labels(SHAPE[0], SHAPE[2:], 3).to(DEV)
        out.append((x, y.flip(1) if i % 2 else y))
    return out


def _train_setup():
    torch.manual_seed(3)
    model = network.ResUnet3D(2, 32, 1, 3, deep_supervision=2).to(DEV)      # Dropout3d on
    network.set_compute_dtype(model, torch.bfloat16)
    model.train()
    ops._drop_counter[0] = 0
    return model, optim.Adam(model.parameters(), lr=1e-3), L.DeepSupervisionLoss(L.HybirdLoss())


def test_graphed_deep_supervision_step_equals_eager():
    batches = _batches(5)
    model_e, opt_e, crit_e = _train_setup()
    losses_e = []
    for x, y in batches:
        opt_e.zero_grad(set_to_none=True)
        loss = crit_e(model_e(x), y)
        loss.backward()
        opt_e.step()
        losses_e.append(loss.detach().clone())
    torch.cuda.synchronize()
    losses_e = [float(v) for v in losses_e]
    levels_e = crit_e.last_level_losses.clone()
    model_g, opt_g, crit_g = _train_setup()
    step = graph.GraphedTrainStep(model_g, crit_g, opt_g, warmup=2)
    losses_g = []
    for x, y in batches:
        losses_g.append(step(x, y).clone())
        assert torch.is_tensor(step.logits) and tuple(step.logits.shape) == (2, 3, 16, 16, 16)
        assert step.logits.dtype == torch.float32
    torch.cuda.synchronize()
    losses_g = [float(v) for v in losses_g]
    assert step.replays == 3 and step.eager_steps == 2
    assert losses_g == losses_e, (losses_g, losses_e)
    assert torch.equal(crit_g.last_level_losses, levels_e)
    bad = [k for (k, a), (_, b) in zip(model_e.state_dict().items(), model_g.state_dict().items()) if not torch.equal(a, b)]
    assert not bad, bad
    assert "net.ds_heads.0.weight" in model_g.state_dict()
    # the level weights are read from device memory: the next replay follows set_weights without a recapture
    x, y = batches[0]
    crit_g.set_weights([1.0, 0.0])
    only_main = float(step(x, y).clone())
    assert step.replays == 4
    lv = crit_g.last_level_losses.clone()
    assert abs(only_main - float(lv[0])) <= 1e-6 * max(1.0, abs(only_main))
    step.release()


# ------------------------------------------------------------------------------------------------ Trainer
class _Cases(torch.utils.data.Dataset):
    def __init__(self, n):
        self.items = []
        for i in range(n):
            y = O.phantom_labels(1, SHAPE[2:], 3)[0]
            self.items.append({"image": O.synth_image((1,) + SHAPE[1:], 500 + i)[0], "label": y.flip(0) if i % 2 else y})

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]


def test_trainer_epoch_validation_and_checkpoint(tmp_path):
    def build(seed):
        torch.manual_seed(seed)
        model = network.ResUnet3D(2, 8, 1, 3, deep_supervision=2).to(DEV)
        return model, optim.Adam(model.parameters(), lr=1e-3)

    model, opt = build(0)
    crit = L.DeepSupervisionLoss(L.HybirdLoss())
    seen = []

    def metric(pred, target):      # metric functions see the full-resolution tensor in both loops
        seen.append((torch.is_tensor(pred), tuple(pred.shape)))
        return L.Dice()(pred, target)

    torch.manual_seed(11)
    np.random.seed(11)
    tr = T.Trainer(model=model, optimizer=opt, loss=crit, dataset=_Cases(2), batch_size=1, valid_split=0.5,
                   dataloader_kwargs={"num_workers": 0}, metrics={"dice": metric}, progress=False)
    assert len(tr.train_indices) == 1 and len(tr.valid_indices) == 1
    save = str(tmp_path / "ds")
    best = tr.fit(num_epochs=1, save_dir=save)
    torch.cuda.synchronize()
    assert np.isfinite(best["loss"]) and "dice" in best
    assert len(seen) == 2 and all(ok and shape == (1, 3, 16, 16, 16) for ok, shape in seen)
    assert not model.training      # the last loop was the validation: eval mode, a single tensor, the same criterion
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    assert "net.ds_heads.0.weight" in sd
    model2, opt2 = build(5)
    tr2 = T.Trainer(model=model2, optimizer=opt2, loss=L.DeepSupervisionLoss(L.HybirdLoss()), dataset=_Cases(2),
                    batch_size=1, valid_split=0.5, dataloader_kwargs={"num_workers": 0}, progress=False)
    tr2.load_checkpoint(save + "-last.pt")
    assert tr2.current_epoch == 1
    assert all(torch.equal(v, model2.state_dict()[k]) for k, v in sd.items())
    # a checkpoint written without the aux heads loads into everything but them
    plain = network.ResUnet3D(2, 8, 1, 3).to(DEV)
    missing = model2.load_state_dict(plain.state_dict(), strict=False)
    assert sorted(missing.missing_keys) == ["net.ds_heads.0.bias", "net.ds_heads.0.weight"] and not missing.unexpected_keys
