"""The 1x1x1 head riding in the last decoder ResBlock (reference network.py:403-416 followed by :547 `fc`).

Forward: ru3d_skip1x1_in_lrelu_head_fwd hands out the head's fp32 logits from the tail kernel's epilogue; z and the logits
are bit for bit what ru3d_skip1x1_in_lrelu_fwd followed by the head's own conv give (same operands, same summation tree).
Backward: ru3d_head_in_bwd never stores the head's input gradient dz: the head's dW / db come from ru3d_head_bwd's pass
without its store, and the reduction pass of the block's InstanceNorm + LeakyReLU backward forms dz in registers.  The
chunk partition and every summation order are those of ru3d_head_bwd + ru3d_in_lrelu_bwd, so EVERYTHING is asserted bit
for bit: g', dW, db, gpre_sum (the skip conv's bias gradient), dy2 and every gradient behind them - a training run is the
same run with the head in the block or behind it.  The float64 CPU reference built from the same stored tensors, under
    err_fused <= 1.5 * err_unfused + 1 ulp of the storage type (of the reference's largest magnitude),
stays as the check that both are right.  The two means m1 / m2 themselves stay in the library's workspace; they are
checked through gpre_sum (V * sum_n m1) and dy2 (scale * (g' - m1 - xhat * m2)), which read them element by element.
Run with `-m gpu`.  ops.skip1x1_in_lrelu_head_fwd asks ru3d_skip1x1_in_lrelu_head_fwd_supported first."""
import functools
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no HIP device", allow_module_level=True)

import _native as N  # noqa: E402
import _ops as ops  # noqa: E402
import graph  # noqa: E402
import loss as L  # noqa: E402
import network  # noqa: E402
import optim  # noqa: E402
from oracle import unet_oracle as O  # noqa: E402

DEV = torch.device("cuda:0")
DTYPES = [torch.bfloat16, torch.float16]
ULP = {torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10}      # spacing of the storage type relative to a value in [1, 2)
SLOPE = 0.01

# (cin, cout, head cout, n, dims, split x): both channel pairs, head widths 1 / 3 / 4, x dense and as the two planes of
# the level-0 concat, three samples (a workgroup meets the sample boundary at another step of its round in every block),
# and one shape with more voxels than one round of the 2048-workgroup grid covers (a second, partly empty round).
# N * V = 65536 is the smallest volume the tail kernel takes.
CASES = [(64, 32, 3, 2, (32, 32, 32), False), (64, 32, 1, 2, (16, 32, 64), True), (64, 32, 4, 2, (32, 32, 32), True),
         (128, 64, 3, 2, (32, 32, 32), False), (128, 64, 4, 2, (16, 32, 64), False), (64, 32, 3, 3, (32, 32, 32), False),
         (64, 32, 3, 2, (64, 64, 96), True)]
IDS = ["%dto%d-h%d-n%d-%s%s" % (c[0], c[1], c[2], c[3], "x".join(map(str, c[4])), "-split" if c[5] else "") for c in CASES]


@pytest.fixture(autouse=True)
def _switch(monkeypatch):
    monkeypatch.delenv("RU3D_HEAD_TAIL", raising=False)


@functools.lru_cache(maxsize=None)
def _case(dt, cin, cout, hc, n, dims, split):
    """Inputs of one case on the device, and the unfused path's results (computed once, never modified).  The samples have
    clearly different statistics and means far from zero, so a workgroup that mixed two samples' sums would show."""
    g = torch.Generator().manual_seed(cin + 7 * hc + n + sum(dims) + int(split))
    d, h, w = dims
    mu_x = torch.tensor([3.0, -5.0, 0.7])[:n].view(n, 1, 1, 1, 1)
    sd_x = torch.tensor([1.0, 4.0, 0.3])[:n].view(n, 1, 1, 1, 1)
    xv = torch.randn(n, cin, d, h, w, generator=g) * sd_x + mu_x
    mu_y = torch.tensor([7.0, -4.0, 20.0])[:n].view(n, 1, 1, 1, 1)
    sd_y = torch.tensor([2.0, 0.5, 5.0])[:n].view(n, 1, 1, 1, 1)
    yv = torch.randn(n, cout, d, h, w, generator=g) * sd_y + mu_y + torch.randn(1, cout, 1, 1, 1, generator=g)
    ws = torch.randn(cout, cin, 1, 1, 1, generator=g) * (1.0 / cin ** 0.5)
    bs = torch.randn(cout, generator=g)
    hw = (torch.randn(hc, cout, 1, 1, 1, generator=g) * 0.3).to(DEV)
    hb = torch.randn(hc, generator=g).to(DEV)
    gv = torch.randn(n, hc, d, h, w, generator=g) * 1e-2 * sd_x + 3e-3
    if split:
        buf = ops.as_input(torch.cat((xv[:, :cin // 2], xv[:, cin // 2:]), dim=0).to(DEV), dt)
        x = N.Split(buf)
    else:
        x = ops.as_input(xv.to(DEV), dt)
    y2 = ops.as_input(yv.to(DEV), dt)
    mean, scale = ops.in_stats(y2)
    pws = ops.pack_weight(ws.to(DEV), N.ROLE_CONV_FWD, dt, 1)
    bs = bs.to(DEV)
    gy = N.to_ndhwc(gv.to(DEV))          # fp32, channels last: how the loss kernel leaves dlogits
    # today's path: tail kernel, then the head as a conv of its own; head backward, then the norm backward
    z = ops.skip1x1_in_lrelu_fwd(x, pws, bs, y2, mean, scale)
    assert z is not None
    logits = ops.ConvFn.apply(z, hw, hb, 1, dt, torch.float32, False, False)
    gz, dw, db = ops.head_bwd(z, gy, hw, True)
    dy, gpre, gsum = ops.in_lrelu_bwd(gz, z, y2, mean, scale, want_gpre=True, want_gpre_sum=True)
    torch.cuda.synchronize()
    return dict(x=x, y2=y2, mean=mean, scale=scale, pws=pws, bs=bs, hw=hw, hb=hb, gy=gy, z=z, logits=logits, dw=dw, db=db,
                dy=dy, gpre=gpre, gsum=gsum)


def _rule(fused, unfused, ref, dt, what):
    """err_fused <= 1.5 err_unfused + 1 ulp of the storage type; the figures are printed before the assertion."""
    ref = ref.double().cpu()
    ef = (fused.detach().double().cpu() - ref).abs().max().item()
    eu = (unfused.detach().double().cpu() - ref).abs().max().item()
    lim = 1.5 * eu + ULP[dt] * ref.abs().max().item()
    print("%s: err fused %.4e  unfused %.4e  limit %.4e  max|ref| %.4e" % (what, ef, eu, lim, ref.abs().max().item()))
    assert ef <= lim, "%s: fused error %.4e > %.4e (unfused %.4e)" % (what, ef, lim, eu)


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_forward_logits_and_z_are_todays_bits(dt, case):
    c = _case(dt, *case)
    hp = ops.pack_weights([(c["hw"], N.ROLE_CONV_FWD, 1, 0, 0)], dt)[0]
    with ops.launch_log() as log:
        both = ops.skip1x1_in_lrelu_head_fwd(c["x"], c["pws"], c["bs"], c["y2"], c["mean"], c["scale"], hp, c["hb"], case[2])
    assert both is not None, "no fused kernel"
    assert log.names == ["skip1x1_in_lrelu_head_fwd"], log.names
    z, logits = both
    assert logits.dtype == torch.float32 and tuple(logits.shape) == tuple(c["logits"].shape)
    assert torch.equal(z, c["z"]), "z differs from the tail kernel's"
    assert torch.equal(logits, c["logits"]), "logits differ from the head kernel's: max %g" % (
        (logits - c["logits"]).abs().max().item())
    # without a bias the head adds 0.0f, as head_fwd_kernel does
    z0, l0 = ops.skip1x1_in_lrelu_head_fwd(c["x"], c["pws"], c["bs"], c["y2"], c["mean"], c["scale"], hp, None, case[2])
    assert torch.equal(l0, ops.ConvFn.apply(c["z"], c["hw"], None, 1, dt, torch.float32, False, False))


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_backward_op(dt, case):
    cin, cout, hc, n, dims, split = case
    c = _case(dt, *case)
    with ops.launch_log() as log:
        out = ops.head_in_bwd(c["z"], c["gy"], c["hw"], True, c["y2"], c["mean"], c["scale"])
    assert out is not None, "no fused kernel"
    assert log.names == ["head_bwd_wgrad", "head_bwd_finalize", "head_in_bwd_reduce", "head_in_bwd_finalize",
                         "head_in_bwd_apply"], log.names
    dy, gpre, gsum, dw, db = out
    assert torch.equal(gpre, c["gpre"]), "g' differs"
    assert torch.equal(dw, c["dw"]), "head dW differs: max %g" % (dw - c["dw"]).abs().max().item()
    assert torch.equal(db, c["db"]), "head db differs"
    assert torch.equal(gsum, c["gsum"]), "gpre_sum differs (same chunks, same order: the same bits)"
    assert torch.equal(dy, c["dy"]), "dy2 differs"
    # float64 reference of what follows from the stored g': the two means, the bias gradient, dy2
    V = dims[0] * dims[1] * dims[2]
    gp = c["gpre"].double().cpu()
    mean = c["mean"].double().cpu().view(n, cout, 1, 1, 1)
    scale = c["scale"].double().cpu().view(n, cout, 1, 1, 1)
    xh = (c["y2"].double().cpu() - mean) * scale
    m1 = gp.mean(dim=(2, 3, 4), keepdim=True)
    m2 = (gp * xh).mean(dim=(2, 3, 4), keepdim=True)
    _rule(gsum, c["gsum"], (m1 * V).sum(dim=0).view(-1), dt, "gpre_sum")
    _rule(dy, c["dy"], scale * (gp - m1 - xh * m2), dt, "dy2")
    # no gradient of the logits: exact zeros everywhere, whatever the sign bits
    zero = ops.head_in_bwd(c["z"], torch.zeros_like(c["gy"]), c["hw"], True, c["y2"], c["mean"], c["scale"])
    assert all(float(t.abs().max()) == 0.0 for t in zero)


def _block(cin, cout, hc, seed):
    torch.manual_seed(seed)
    blk = network.ResBlock(cin, cout).to(DEV)
    fc = torch.nn.Conv3d(cout, hc, kernel_size=1).to(DEV)
    blk.eval()          # Dropout3d off: the two runs see the same function
    return blk, fc


# the float64 CPU reference of the 128 -> 64 block costs four times the 64 -> 32 one's: once, in the benchmarked type
@pytest.mark.parametrize("dt,cin,cout,hc,dims", [(torch.bfloat16, 64, 32, 3, (32, 32, 32)), (torch.float16, 64, 32, 3, (32, 32, 32)),
                                                 (torch.bfloat16, 128, 64, 1, (16, 32, 64))],
                         ids=["bf16-64to32", "fp16-64to32", "bf16-128to64"])
def test_block_with_and_without_head(dt, cin, cout, hc, dims, monkeypatch):
    """ResBlock.forward(x, head=fc) against the block followed by the head's ConvFn: logits bit-equal, the head's gradients
    bit-equal, every gradient behind the InstanceNorm backward's means under the rule, against float64 autograd on the CPU
    through the same function of the stored (rounded) input."""
    n = 2
    d, h, w = dims
    g = torch.Generator().manual_seed(cin + hc)
    xv = torch.randn(n, cin, d, h, w, generator=g) * torch.tensor([1.0, 3.0]).view(2, 1, 1, 1, 1) \
        + torch.tensor([2.0, -6.0]).view(2, 1, 1, 1, 1)
    gv = torch.randn(n, hc, d, h, w, generator=g) * 1e-2 + 2e-3
    blk, fc = _block(cin, cout, hc, 11)
    params = [blk.conv1.weight, blk.conv2.weight, blk.skip_conv.weight, blk.skip_conv.bias, fc.weight, fc.bias]
    names = ["gw1", "gw2", "gws", "gbs", "head dW", "head db"]
    gy = N.to_ndhwc(gv.to(DEV))
    calls = []
    real = ops.head_in_bwd
    monkeypatch.setattr(ops, "head_in_bwd", lambda *a, **k: calls.append(real(*a, **k)) or calls[-1])

    def run(fused):
        x = ops.as_input(xv.to(DEV), dt).requires_grad_(True)
        for p in params:
            p.grad = None
        if fused:
            assert blk.takes_head(x, fc)
            logits = blk(x, head=fc)
        else:
            monkeypatch.setenv("RU3D_HEAD_TAIL", "0")
            assert not blk.takes_head(x, fc)
            monkeypatch.delenv("RU3D_HEAD_TAIL")
            logits = ops.ConvFn.apply(blk(x), fc.weight, fc.bias, 1, dt, torch.float32, False, False)
        logits.backward(gy)
        torch.cuda.synchronize()
        return logits.detach(), [x.grad] + [p.grad.clone() for p in params]

    l_u, g_u = run(False)
    assert not calls
    l_f, g_f = run(True)
    assert len(calls) == 1 and calls[0] is not None, "the fused backward did not run"
    assert torch.equal(l_f, l_u), "logits differ"
    assert torch.equal(g_f[5], g_u[5]) and torch.equal(g_f[6], g_u[6]), "the head's gradients differ"
    # float64 reference
    F = torch.nn.functional
    xr = xv.to(dt).double().requires_grad_(True)
    pr = [p.detach().double().cpu().requires_grad_(True) for p in params]
    b1, b2 = blk.conv1.bias.detach().double().cpu(), blk.conv2.bias.detach().double().cpu()
    y = F.leaky_relu(F.instance_norm(F.conv3d(xr, pr[0], b1, padding=1)), SLOPE)
    y = F.instance_norm(F.conv3d(y, pr[1], b2, padding=1)) + F.conv3d(xr, pr[2], pr[3])
    ref_logits = F.conv3d(F.leaky_relu(y, SLOPE), pr[4], pr[5])
    ref_logits.backward(gv.double())
    refs = [xr.grad] + [p.grad for p in pr]
    for name, gf, gu, r in zip(["gx"] + names, g_f, g_u, refs):
        assert torch.equal(gf, gu), "%s differs from the two-node path" % name
        _rule(gf, gu, r, dt, name)


def _net(dt, seed=5):
    torch.manual_seed(seed)
    model = network.ResUnet3D(1, 32, 1, 3).to(DEV)
    network.set_compute_dtype(model, dt)
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout3d):
            m.p = 0.0          # no draw: the float64 oracle sees the same function
    model.train()
    return model


def _batch(seed):
    x = O.synth_image((2, 1, 32, 32, 32), seed)
    y = O.phantom_labels(2, (32, 32, 32), 3)
    return x, y


def _one_step(dt, fused, monkeypatch):
    if not fused:
        monkeypatch.setenv("RU3D_HEAD_TAIL", "0")
    model = _net(dt)
    x, y = _batch(21)
    with ops.launch_log() as log:
        logits = model(x.to(DEV))
    assert ("skip1x1_in_lrelu_head_fwd" in log.names) == fused and ("head_fwd" in log.names) != fused, log.names
    lval = L.HybirdLoss()(logits, y.to(DEV))
    lval.backward()
    torch.cuda.synchronize()
    monkeypatch.delenv("RU3D_HEAD_TAIL", raising=False)
    return model, logits.detach(), lval.detach(), {k: p.grad for k, p in model.named_parameters() if p.grad is not None}


def test_net_fused_equals_switch_off(monkeypatch):
    """ResUnet3D(1, 32, 1, 3) on 2 x 1 x 32^3, one training step with the head in the last block and with RU3D_HEAD_TAIL=0
    in the same process: logits and loss bit-equal, every parameter gradient under the rule against the float64 oracle."""
    dt = torch.bfloat16
    m_u, l_u, loss_u, g_u = _one_step(dt, False, monkeypatch)
    m_f, l_f, loss_f, g_f = _one_step(dt, True, monkeypatch)
    assert torch.equal(l_f, l_u) and torch.equal(loss_f, loss_u)
    assert sorted(g_f) == sorted(g_u)
    assert torch.equal(g_f["net.fc.weight"], g_u["net.fc.weight"]) and torch.equal(g_f["net.fc.bias"], g_u["net.fc.bias"])
    x, y = _batch(21)
    w = {k: v.detach().double().cpu() for k, v in m_f.state_dict().items()}
    _, _, ref = O.train_step(w, x.double(), y, 1)
    checked = 0
    for k in sorted(g_f):
        if k in ref:
            assert torch.equal(g_f[k], g_u[k]), k
            _rule(g_f[k], g_u[k], ref[k], dt, k)
            checked += 1
    assert checked == len(g_f) >= 16, (checked, len(g_f))      # every parameter that has a gradient has a reference


@pytest.mark.parametrize("half", ["fwd", "bwd"])
def test_switch_fuses_one_half(half, monkeypatch):
    """RU3D_HEAD_TAIL=fwd / bwd (the A/B of the halves): the head stays in the block's node, only that half runs the fused
    kernel; logits, loss and the head's gradients are the fused path's bits."""
    dt = torch.bfloat16
    m_f, l_f, loss_f, g_f = _one_step(dt, True, monkeypatch)
    calls = []
    real = ops.head_in_bwd
    monkeypatch.setattr(ops, "head_in_bwd", lambda *a, **k: calls.append(real(*a, **k)) or calls[-1])
    monkeypatch.setenv("RU3D_HEAD_TAIL", half)
    model = _net(dt)
    x, y = _batch(21)
    with ops.launch_log() as log:
        logits = model(x.to(DEV))
    assert ("skip1x1_in_lrelu_head_fwd" in log.names) == (half == "fwd") and ("head_fwd" in log.names) == (half == "bwd")
    lval = L.HybirdLoss()(logits, y.to(DEV))
    lval.backward()
    torch.cuda.synchronize()
    assert len(calls) == (1 if half == "bwd" else 0)
    assert torch.equal(logits.detach(), l_f) and torch.equal(lval.detach(), loss_f)
    for k in ("net.fc.weight", "net.fc.bias"):
        assert torch.equal(dict(model.named_parameters())[k].grad, g_f[k]), k


def test_net_graph_replay_equals_eager():
    """Four steps, two of them hipGraph replays, leave the eager loop's losses and weights: the fused entry points make no
    host synchronisation and no address changes between replays."""
    dt = torch.bfloat16

    def run(graphed):
        model = _net(dt, seed=6)
        opt = optim.Adam(model.parameters(), lr=1e-3)
        crit = L.HybirdLoss()
        step = graph.GraphedTrainStep(model, crit, opt, warmup=2) if graphed else None
        losses = []
        for i in range(4):
            x, y = _batch(30 + i)
            x, y = x.to(DEV), y.to(DEV)
            if graphed:
                losses.append(float(step(x, y)))
            else:
                opt.zero_grad(set_to_none=True)
                lv = crit(model(x), y)
                lv.backward()
                opt.step()
                losses.append(float(lv.detach()))
        torch.cuda.synchronize()
        if graphed:
            assert step.replays == 2
            step.release()
        return model, losses

    m_e, l_e = run(False)
    m_g, l_g = run(True)
    assert l_e == l_g, (l_e, l_g)
    bad = [k for (k, a), (_, b) in zip(m_e.state_dict().items(), m_g.state_dict().items()) if not torch.equal(a, b)]
    assert not bad, bad


def test_eval_forward_takes_the_fused_kernel():
    model = _net(torch.bfloat16)
    model.eval()
    x, _ = _batch(40)
    with torch.no_grad():
        with ops.launch_log() as log:
            a = model(x.to(DEV))
        os.environ["RU3D_HEAD_TAIL"] = "0"
        try:
            b = model(x.to(DEV))
        finally:
            del os.environ["RU3D_HEAD_TAIL"]
    assert "skip1x1_in_lrelu_head_fwd" in log.names and "head_fwd" not in log.names, log.names
    assert torch.equal(a, b)


@pytest.mark.parametrize("what", ["cout5", "fp32", "checkpoint"])
def test_fallbacks_take_todays_path(what):
    """Five classes, fp32 parity mode and checkpointed blocks keep the head a launch of its own and give the results of
    RU3D_HEAD_TAIL=0."""
    def run(switch_off):
        torch.manual_seed(8)
        model = network.ResUnet3D(1, 32, 1, 5 if what == "cout5" else 3).to(DEV)
        network.set_compute_dtype(model, torch.float32 if what == "fp32" else torch.bfloat16)
        for m in model.modules():
            if isinstance(m, torch.nn.Dropout3d):
                m.p = 0.0
        if what == "checkpoint":
            network.set_checkpointing(model, True)
        model.train()
        x, y = _batch(50)
        if switch_off:
            os.environ["RU3D_HEAD_TAIL"] = "0"
        try:
            with ops.launch_log() as log:
                logits = model(x.to(DEV))
            lval = L.HybirdLoss()(logits, (y % (5 if what == "cout5" else 3)).to(DEV))
            lval.backward()
            torch.cuda.synchronize()
        finally:
            os.environ.pop("RU3D_HEAD_TAIL", None)
        return log.names, logits.detach(), {k: p.grad for k, p in model.named_parameters() if p.grad is not None}

    names, logits, grads = run(False)
    assert "skip1x1_in_lrelu_head_fwd" not in names, names
    names0, logits0, grads0 = run(True)
    assert names == names0
    if what == "fp32":      # the parity-mode kernels sum some gradients with float atomics: equal run to run only in value
        assert torch.allclose(logits, logits0, rtol=1e-5, atol=1e-6)
    else:
        assert torch.equal(logits, logits0)
        for k in grads:
            assert torch.equal(grads[k], grads0[k]), k
