"""The plain 3D U-Net on the native path: 2x2x2 max pooling (csrc/pool.hip) held bit for bit against torch's CPU
max_pool3d, ConvBlock stacks (ops.ConvStackFn) against float64 copies of the torch modules, the whole net against the
reference's own numbers (tests/golden/make_golden_plain.py), mixed ConvBlock / ResBlock / MaxPoolBlock chains against
their RU3D_PLAIN_BLOCKS=torch run, 16-bit storage, deep supervision and the captured training step.
Run with `-m gpu`."""
import copy
import os

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
from oracle import unet_oracle as O  # noqa: E402

DEV = torch.device("cuda:0")
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
INT_VIEW = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}

# (shape [N, C, D, H, W], channels of the buffer the operand is a slice of, first channel of the slice)
POOL_CASES = [
    ((1, 8, 4, 4, 4), 8, 0),          # base case
    ((2, 5, 6, 10, 4), 5, 0),         # channel count no multiple of the vector width: element-per-lane kernels
    ((1, 32, 5, 7, 9), 32, 0),        # odd extents: floored, trailing planes
    ((2, 64, 8, 6, 12), 64, 0),       # wide channels, more than one block
    ((1, 16, 4, 6, 4), 24, 0),        # buf[:, :16] of a 24-channel buffer: ld > c, still 16-byte steps
    ((1, 8, 4, 4, 6), 20, 4),         # buf[:, 4:12] of a 20-channel buffer: pointer and pitch off the 16-byte grid
]
POOL_IDS = ["base", "scalar", "odd", "wide", "slice", "misaligned"]


def _count_calls(fn_cls):
    calls = []
    orig = fn_cls.apply
    fn_cls.apply = staticmethod(lambda *a: (calls.append(1), orig(*a))[1])
    return calls, (lambda: setattr(fn_cls, "apply", orig))


# --------------------------------------------------------------------------- pooling kernel
def _pool_operand(case, dtype, seed, nans=False):
    """(operand on the device, the same values float32 NCDHW-contiguous on the CPU).  round(2 * randn) / 2: many ties
    and both signed zeros, every value exact in all three storage types."""
    (n, c, d, h, w), cbuf, c0 = case
    g = torch.Generator().manual_seed(seed)
    v = torch.round(2 * torch.randn((n, d, h, w, cbuf), generator=g)) / 2
    if nans:
        v[torch.rand(v.shape, generator=g) < 0.15] = float("nan")      # several in some windows, none in others
    buf = v.to(dtype).to(DEV).permute(0, 4, 1, 2, 3)
    x = buf[:, c0:c0 + c]
    return x, x.float().cpu().contiguous()


def _expected(xc):
    """torch's CPU pooling of the float32 upcast (exact and order preserving): values and winner codes dz*4+dy*2+dx."""
    want, flat = F.max_pool3d(xc, 2, 2, return_indices=True)
    _, _, d, h, w = xc.shape
    od, oh, ow = want.shape[2:]
    zz = flat // (h * w) - 2 * torch.arange(od).view(1, 1, od, 1, 1)
    yy = (flat // w) % h - 2 * torch.arange(oh).view(1, 1, 1, oh, 1)
    xx = flat % w - 2 * torch.arange(ow).view(1, 1, 1, 1, ow)
    assert int(zz.min()) >= 0 and int(zz.max()) <= 1 and int(yy.min()) >= 0 and int(yy.max()) <= 1
    return want, (zz * 4 + yy * 2 + xx).to(torch.uint8)


def _assert_pool_fwd(case, dtype, nans):
    x, xc = _pool_operand(case, dtype, 5, nans)
    want, codes = _expected(xc)
    with ops.launch_log() as log:
        y, idx = ops.maxpool_fwd(x, want_idx=True)
    assert log.names == ["maxpool3d_fwd"]
    assert tuple(y.shape) == tuple(want.shape) and y.dtype == dtype
    iv = INT_VIEW[dtype]
    assert torch.equal(y.cpu().contiguous().view(iv), want.to(dtype).contiguous().view(iv))
    assert torch.equal(idx.permute(0, 4, 1, 2, 3).cpu(), codes)
    y2, none = ops.maxpool_fwd(x, want_idx=False)          # inference: no codes, the same values
    assert none is None and torch.equal(y2.contiguous().view(iv), y.contiguous().view(iv))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("case", POOL_CASES, ids=POOL_IDS)
def test_maxpool_forward_is_torchs_bit_for_bit(case, dtype):
    _assert_pool_fwd(case, dtype, nans=False)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("case", [POOL_CASES[2], POOL_CASES[1]], ids=["odd", "scalar"])
def test_maxpool_forward_with_nans(case, dtype):
    """Every NaN replaces the running maximum: the LAST NaN of a window wins and the output is NaN."""
    _assert_pool_fwd(case, dtype, nans=True)


def _assert_same_gradient(dx, want, dtype):
    """Exact equality of every value (a NaN left from the pre-fill fails it), and of every bit where the value is not
    zero.  The one place the bits may differ: torch ADDS dy into a zeroed tensor, which turns a gradient of -0.0 into
    +0.0, where the kernel stores the copy."""
    got = dx.cpu().contiguous()
    want = want.contiguous()
    assert torch.equal(got, want)
    iv = INT_VIEW[dtype]
    assert torch.equal(got.view(iv)[want != 0], want.view(iv)[want != 0])


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("case", POOL_CASES, ids=POOL_IDS)
def test_maxpool_backward_is_torchs_and_writes_every_element(case, dtype):
    x, xc = _pool_operand(case, dtype, 6)
    (n, c, d, h, w), cbuf, c0 = case
    y, idx = ops.maxpool_fwd(x, want_idx=True)
    g = torch.Generator().manual_seed(7)
    gy = (torch.round(4 * torch.randn(tuple(y.shape), generator=g)) / 4).to(dtype)
    xr = xc.clone().requires_grad_(True)
    F.max_pool3d(xr, 2, 2).backward(gy.float())
    want = xr.grad.to(dtype)                                # copies or zeros: exact, zero trailing planes included
    # the gradient goes into a NaN-filled slice of a wider buffer: every element of the slice is written, none beyond
    buf = torch.full((n, d, h, w, cbuf), float("nan"), dtype=dtype, device=DEV).permute(0, 4, 1, 2, 3)
    dx = buf[:, c0:c0 + c]
    gyd = N.to_ndhwc(gy.to(DEV))
    ddy, ddx = N.desc(gyd), N.desc(dx)
    with ops.launch_log() as log:
        N.check(N.lib.ru3d_maxpool3d_bwd(N.ref(ddy), N.ptr(idx), N.ref(ddx), N.dtype_code(dtype), N.stream()), "bwd")
    assert log.names == ["maxpool3d_bwd"]
    _assert_same_gradient(dx, want, dtype)
    rest = torch.cat((buf[:, :c0], buf[:, c0 + c:]), dim=1)
    assert bool(torch.isnan(rest).all())
    # and the wrapper, which allocates the gradient itself
    dx2 = ops.maxpool_bwd(gyd, idx, (n, c, d, h, w))
    _assert_same_gradient(dx2, want, dtype)


def test_maxpool_rejects_what_it_does_not_take():
    x = N.new_act(1, 8, 4, 4, 1, torch.float32, DEV, zero=True)
    with pytest.raises(N.Ru3dError, match="at least 2"):
        ops.maxpool_fwd(x)
    y = N.new_act(1, 8, 2, 2, 1, torch.float32, DEV)       # the library's own check, whatever the caller allocated
    dx, dy = N.desc(x), N.desc(y)
    assert N.lib.ru3d_maxpool3d_fwd(N.ref(dx), N.ref(dy), None, N.F32, N.stream()) < 0
    assert "at least 2" in N.lib.ru3d_last_error().decode()
    x = N.new_act(2, 8, 4, 4, 4, torch.bfloat16, DEV, zero=True)
    y = N.new_act(1, 16, 2, 2, 2, torch.bfloat16, DEV)
    dx, dy = N.Split(x).desc(), N.desc(y)
    assert N.lib.ru3d_maxpool3d_fwd(N.ref(dx), N.ref(dy), None, N.BF16, N.stream()) < 0
    assert "split" in N.lib.ru3d_last_error().decode()


def test_maxpool_element_offsets_beyond_2_to_31():
    """64-bit offsets: the last planes of a tensor of more than 2^31 elements pool to what the same planes give as a
    small tensor of their own, forward and backward."""
    n, c, d, h, w = 1, 64, 258, 258, 512
    assert n * c * d * h * w > (1 << 31)
    x = torch.empty((n, d, h, w, c), dtype=torch.bfloat16, device=DEV).normal_().permute(0, 4, 1, 2, 3)
    y, idx = ops.maxpool_fwd(x)
    tail = x[:, :, -2:]
    yt, it = ops.maxpool_fwd(tail)
    assert torch.equal(y[:, :, -1:].view(torch.int16), yt.view(torch.int16)) and torch.equal(idx[:, -1:], it)
    gy = torch.empty_like(y).normal_()
    dx = ops.maxpool_bwd(gy, idx, (n, c, d, h, w))
    dt = ops.maxpool_bwd(N.to_ndhwc(gy[:, :, -1:]), it, tuple(tail.shape))
    assert torch.equal(dx[:, :, -2:].view(torch.int16), dt.view(torch.int16))
    assert int(dx[:, :, -2:].count_nonzero()) == int(gy[:, :, -1:].count_nonzero()) > 0


# --------------------------------------------------------------------------- ConvBlock stacks
def _masks(blocks, n, drop):
    keeps = []
    for b in blocks:
        keep = None
        if drop:
            keep = (torch.rand(n, b.out_channels, device=DEV) > 0.4).float()
            keep[0, 0] = 0.0
            keep[1, 0] = 1.0
            b._forced_keep = keep
        keeps.append(keep)
    return keeps


def _stack_oracle(blocks, x, keeps, p):
    """float64 CPU copies of the torch modules, the recorded Dropout3d masks applied by hand."""
    refs = [copy.deepcopy(b).cpu().double() for b in blocks]
    xr = x.detach().cpu().double().requires_grad_(True)
    h = xr
    for r, keep in zip(refs, keeps):
        h = r.conv(h)
        if keep is not None:
            h = h * (keep.cpu().double() / (1.0 - p))[:, :, None, None, None]
        h = F.leaky_relu(r.norm(h), 0.01)
    return refs, xr, h


def _assert_param_grads(pairs):
    for k, pn, pr in pairs:
        if k.endswith("conv.bias") and pn.grad is None:      # straight in front of an InstanceNorm: analytically zero
            assert pr.grad.abs().max().item() < 1e-9, k
            continue
        assert pn.grad is not None, k
        scale = max(pr.grad.abs().max().item(), 1e-3)
        assert (pn.grad.cpu().double() - pr.grad).abs().max().item() <= 5e-3 * scale, k


@pytest.mark.parametrize("cin,cout,stacks,drop,dims", [(8, 16, 2, True, (12, 10, 8)), (24, 8, 2, False, (6, 10, 4)),
                                                       (4, 4, 1, True, (5, 7, 3)), (16, 16, 3, False, (8, 8, 8))])
def test_conv_block_stack_vs_fp64(cin, cout, stacks, drop, dims):
    torch.manual_seed(11)
    kw = {} if drop else {"dropout_op": None}
    if stacks == 1:
        mod = network.ConvBlock(cin, cout, **kw).to(DEV).train()
        blocks = [mod]
    else:
        mod = network.ConvBlockStack(cin, cout, num_stacks=stacks, **kw).to(DEV).train()
        blocks = list(mod.conv_blocks)
    assert all(b._native for b in blocks)
    n = 3
    keeps = _masks(blocks, n, drop)
    x = torch.randn(n, cin, *dims, device=DEV, requires_grad=True)
    g = torch.randn(n, cout, *dims, device=DEV)
    refs, xr, out_r = _stack_oracle(blocks, x, keeps, 0.5)
    out_r.backward(g.cpu().double())
    calls, undo = _count_calls(ops.ConvStackFn)
    try:
        out = mod(x)
    finally:
        undo()
    assert len(calls) == 1                                  # a stack is one autograd node
    out.backward(g)
    assert (out.detach().cpu().double() - out_r.detach()).abs().max().item() <= 2e-4
    assert (x.grad.cpu().double() - xr.grad).abs().max().item() <= 2e-3 * max(1.0, xr.grad.abs().max().item())
    pairs = []
    for i, (b, r) in enumerate(zip(blocks, refs)):
        assert b.conv.bias.grad is None, i
        pairs += [("%d.conv.weight" % i, b.conv.weight, r.conv.weight), ("%d.conv.bias" % i, b.conv.bias, r.conv.bias)]
    _assert_param_grads(pairs)


def test_res_rec_block_runs_its_conv_blocks_natively():
    """RecBlock applies ONE ConvBlock t + 1 = 3 times: its weight gradient is the sum of the three uses (each from a
    conv_wgrad call without an arena key)."""
    torch.manual_seed(12)
    blk = network.ResRecBlock(4, 8, dropout_op=None).to(DEV).train()
    assert blk.rcnn[0].conv._native and blk.rcnn[0].conv._shared and blk.rcnn[1].conv._shared
    x = torch.randn(2, 4, 8, 6, 4, device=DEV, requires_grad=True)
    g = torch.randn(2, 8, 8, 6, 4, device=DEV)
    ref = copy.deepcopy(blk).cpu().double()                 # CPU tensors take the torch composition
    xr = x.detach().cpu().double().requires_grad_(True)
    out_r = ref(xr)
    out_r.backward(g.cpu().double())
    calls, undo = _count_calls(ops.ConvStackFn)
    try:
        out = blk(x)
    finally:
        undo()
    assert len(calls) == 6                                  # two RecBlocks x three uses
    out.backward(g)
    assert (out.detach().cpu().double() - out_r.detach()).abs().max().item() <= 2e-4
    assert (x.grad.cpu().double() - xr.grad).abs().max().item() <= 2e-3 * max(1.0, xr.grad.abs().max().item())
    _assert_param_grads([(k, pn, pr) for (k, pn), (_, pr) in zip(blk.named_parameters(), ref.named_parameters())])
    assert blk.rcnn[0].conv.conv.weight.grad.abs().max().item() > 0


# --------------------------------------------------------------------------- whole nets
def _zero_dropout(model):
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout3d):
            m.p = 0.0
    return model


def _norm_bias(k):
    """A conv bias straight in front of an InstanceNorm: ConvBlock convs, a ResBlock's conv1 / conv2."""
    return (".conv_blocks." in k and k.endswith(".conv.bias")) or k.endswith(("conv1.bias", "conv2.bias"))


def test_plain_unet_vs_reference(golden_dir):
    """One training forward + backward of the reference's default Unet (ConvBlockStack / MaxPoolBlock,
    generate_paired_features2(2, 8)) against the reference's own numbers: logits, loss, every parameter gradient."""
    z = dict(np.load(os.path.join(golden_dir, "g13_plain.npz")))
    z.update(np.load(os.path.join(golden_dir, "g13_plain_logits.npz")))
    z.update(np.load(os.path.join(golden_dir, "g13_plain_grads.npz")))
    torch.manual_seed(0)
    model = network.Unet(1, 3, network.generate_paired_features2(2, 8))
    model.load_state_dict({k[2:]: torch.from_numpy(v) for k, v in z.items() if k.startswith("w/")}, strict=True)
    model = _zero_dropout(model).to(DEV).train()
    assert model._native_chain() is not None and model._pad is False and model._linked is False
    x = torch.from_numpy(z["x"]).to(DEV)
    y = torch.from_numpy(z["y"].astype(np.int64)).to(DEV)
    counted = [_count_calls(c) for c in (ops.ConvStackFn, ops.MaxPoolFn, ops.UpFn)]
    try:
        logits = model(x)
    finally:
        for _, undo in counted:
            undo()
    assert [len(c) for c, _ in counted] == [5, 2, 2]
    loss = L.HybirdLoss(weight_v=[1, 10, 20])(logits, y)
    loss.backward()
    assert (logits.detach().cpu() - torch.from_numpy(z["logits"])).abs().max().item() <= 2e-4
    assert abs(float(loss.detach()) - float(z["loss"])) <= 1e-5
    checked = 0
    for k, p in model.named_parameters():
        want = torch.from_numpy(z["g/" + k])                # the reference leaves no parameter without a gradient
        if p.grad is None:      # conv bias in front of a norm layer: identically zero gradient
            assert _norm_bias(k) and float(want.abs().max()) < 1e-5, k
            continue
        if _norm_bias(k) and float(want.abs().max()) < 1e-6:
            continue
        err = ((p.grad.cpu() - want).norm() / want.norm().clamp_min(1e-12)).item()
        assert err <= 3e-2, (k, err)
        checked += 1
    assert checked >= 18


def _mixed(which):
    if which == "a":
        return network.Unet(1, 2, network.generate_paired_features(2, 8), pool_block=network.ResBlock,
                            pool_kwargs={'stride': 2}, encode_block=network.ConvBlockStack, decode_block=network.ResBlock)
    if which == "b":
        return network.Unet(1, 2, network.generate_paired_features2(2, 8), encode_block=network.ResBlockStack,
                            decode_block=network.ResBlock)
    return _res_encoder_plain_decoder(8)


def _res_encoder_plain_decoder(feat):
    """ResBlock encoders and pooling - everything the skip-link route asks of a net - around ConvBlockStack decoders."""
    return network.Unet(1, 2, network.generate_paired_features(2, feat), pool_block=network.ResBlock,
                        pool_kwargs={'stride': 2}, encode_block=network.ResBlockStack, decode_block=network.ConvBlockStack)


@pytest.mark.parametrize("which", ["a", "b", "c"])
def test_mixed_chains_native_vs_torch_blocks(which, monkeypatch):
    """ConvBlockStack encoders between ResBlock pooling / decoders (a), ResBlocks around MaxPoolBlock (b), ResBlock
    encoders and pooling with ConvBlockStack decoders (c): native chains, unlinked, and the same numbers as with the plain blocks kept torch modules (RU3D_PLAIN_BLOCKS=torch: native ResBlocks around
    torch blocks, the route these nets took before)."""
    torch.manual_seed(13)
    model = _zero_dropout(_mixed(which)).to(DEV).train()
    assert model._native_chain() is not None and model._in_chain and not model._pad and not model._linked
    x = O.synth_image((2, 1, 32, 32, 32), 5).to(DEV)
    y = O.phantom_labels(2, (32, 32, 32), 2).to(DEV)
    runs = {}
    for mode in ("native", "torch"):
        monkeypatch.setenv("RU3D_PLAIN_BLOCKS", mode)
        model.zero_grad(set_to_none=True)
        counted = [_count_calls(c) for c in (ops.ConvStackFn, ops.MaxPoolFn, ops.ResBlockFn)]
        try:
            logits = model(x)
        finally:
            for _, undo in counted:
                undo()
        got = tuple(len(c) for c, _ in counted)
        nres = {"a": 4, "b": 8, "c": 8}[which]
        want = {"a": (3, 0), "b": (0, 2), "c": (2, 0)}[which] + (nres,) if mode == "native" else (0, 0, nres)
        assert got == want
        L.HybirdLoss()(logits, y).backward()
        runs[mode] = (logits.detach().clone(), {k: (None if p.grad is None else p.grad.clone())
                                                for k, p in model.named_parameters()})
    (ln, gn), (lt, gt) = runs["native"], runs["torch"]
    assert (ln - lt).abs().max().item() <= 2e-4
    checked = 0
    for k, a in gn.items():
        b = gt[k]
        if a is None:           # unused skip conv (both None) or a bias in front of a norm (torch: rounding noise)
            assert b is None or (_norm_bias(k) and b.abs().max().item() < 1e-5), k
            continue
        err = ((a - b).norm() / b.norm().clamp_min(1e-12)).item()
        assert err <= 3e-2, (k, err)
        checked += 1
    assert checked >= 10


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_res_encoder_plain_decoder_trains_in_16_bit(dtype):
    """The mix that meets every condition the skip links put on encoders and pooling blocks: with plain decoders it
    stays unlinked, and a 16-bit training step (Dropout3d on) runs: logits near the fp32 run's, finite gradients."""
    torch.manual_seed(17)
    model = _res_encoder_plain_decoder(32).to(DEV).train()
    x = O.synth_image((2, 1, 32, 32, 32), 23).to(DEV)
    y = O.phantom_labels(2, (32, 32, 32), 2).to(DEV)
    model.eval()
    with torch.no_grad():
        ref = model(x)
    network.set_compute_dtype(model, dtype)
    assert model._native_chain() is not None and model._linked is False and model._storage_dtype() == dtype
    with torch.no_grad():
        got = model(x)
    # the bound of test_attention_gate_16_bit_and_padded for these two storage types
    rel = ((got - ref).float().norm() / ref.float().norm()).item()
    assert rel <= (0.06 if dtype == torch.bfloat16 else 0.008), rel
    model.train()
    counted = [_count_calls(c) for c in (ops.ConvStackFn, ops.ResBlockFn)]
    try:
        logits = model(x)
    finally:
        for _, undo in counted:
            undo()
    assert [len(c) for c, _ in counted] == [2, 8]
    L.HybirdLoss()(logits, y).backward()
    seen = 0
    for k, p in model.named_parameters():
        if p.grad is None:
            assert _norm_bias(k) or "skip_conv" in k, k
            continue
        assert p.grad.shape == p.shape and bool(torch.isfinite(p.grad).all()), k
        seen += 1
    assert seen >= 20


def test_no_grad_forward_saves_nothing(monkeypatch):
    """Under torch.no_grad() with parameters (and an input) that require gradients: no input-gradient weight packs, no
    pooling codes, nothing kept - and the values of the taped forward."""
    torch.manual_seed(18)
    stack = network.ConvBlockStack(4, 8, dropout_op=None).to(DEV).train()
    pool = network.MaxPoolBlock(8, 8)
    x = torch.randn(2, 4, 8, 6, 4, device=DEV, requires_grad=True)
    packs, codes = [], []
    orig_pack, orig_pool = ops.pack_weights, ops.maxpool_fwd
    monkeypatch.setattr(ops, "pack_weights", lambda specs, dt: (packs.append(len(specs)), orig_pack(specs, dt))[1])
    monkeypatch.setattr(ops, "maxpool_fwd", lambda t, want_idx=True: (codes.append(want_idx), orig_pool(t, want_idx))[1])
    taped = pool(stack(x))
    assert packs == [4] and codes == [True] and taped.requires_grad
    with torch.no_grad():
        free = pool(stack(x))
    assert packs == [4, 2] and codes == [True, False] and not free.requires_grad and free.grad_fn is None
    assert torch.equal(free, taped.detach())
    taped.sum().backward()                                   # the taped node is untouched by the call in between
    assert x.grad is not None and stack.conv_blocks[0].conv.weight.grad is not None


def _rel_to_fp32(model, x, dtype):
    with torch.no_grad():
        ref = model(x)
        network.set_compute_dtype(model, dtype)
        got = model(x)
    return ((got - ref).float().norm() / ref.float().norm()).item()


@pytest.mark.parametrize("feat,dtype", [(32, torch.bfloat16), (32, torch.float16), (24, torch.bfloat16)],
                         ids=["32-bf16", "32-fp16", "24-bf16"])
def test_plain_unet_16_bit_storage(feat, dtype):
    """16-bit storage reaches the plain net (before, set_compute_dtype did nothing for it): relative L2 distance of the
    logits to the same model's fp32 native run, held to 1.5 x the same measure of ResUnet3D(2, F, 1, 2) on the same
    input and dtype (the margin: the two nets' conv depths differ).  Measured (profiles/plain_unet_yardstick.txt):
    0.0217 against 0.0170 (F = 32 bf16), 0.0027 against 0.0022 (F = 32 fp16), 0.0233 against 0.0180 (F = 24 bf16).
    Then one training step."""
    torch.manual_seed(14)
    model = network.Unet(1, 2, network.generate_paired_features2(2, feat)).to(DEV).eval()
    yard = network.ResUnet3D(2, feat, 1, 2).to(DEV).eval()
    x = O.synth_image((1, 1, 32, 32, 32), 21).to(DEV)
    rel = _rel_to_fp32(model, x, dtype)
    assert model._storage_dtype() == dtype and model._pad is False
    rel_yard = _rel_to_fp32(yard, x, dtype)
    line = "plain Unet F=%d %s: rel L2 to fp32 %.5f; ResUnet3D(2, %d, 1, 2): %.5f" % (
        feat, str(dtype).replace("torch.", ""), rel, feat, rel_yard)
    print(line)
    out = os.environ.get("RU3D_OUT")      # where the bench tools write too; profiles/plain_unet_yardstick.txt is such a run's file
    if out:
        path = os.path.join(out, "plain_unet_yardstick.txt")
        head = line.split(":")[0] + ":"
        kept = [l for l in (open(path).read().splitlines() if os.path.exists(path) else []) if not l.startswith(head)]
        with open(path, "w") as fh:
            fh.write("\n".join(kept + [line]) + "\n")
    assert rel <= 1.5 * rel_yard, line
    model.train()
    y = O.phantom_labels(1, (32, 32, 32), 2).to(DEV)
    L.HybirdLoss()(model(x), y).backward()
    seen = 0
    for k, p in model.named_parameters():
        if p.grad is None:
            assert _norm_bias(k), k
            continue
        assert p.grad.shape == p.shape and bool(torch.isfinite(p.grad).all()), k
        seen += 1
    assert seen >= 18


def test_plain_unet_eval_equals_train_without_dropout_and_deep_supervision():
    torch.manual_seed(15)
    model = _zero_dropout(network.Unet(1, 3, network.generate_paired_features2(2, 8))).to(DEV).train()
    x = O.synth_image((2, 1, 32, 32, 32), 22).to(DEV)
    train_logits = model(x).detach()
    model.eval()
    with torch.no_grad():
        eval_logits = model(x)
    assert torch.equal(train_logits, eval_logits)
    ds = network.Unet(1, 3, network.generate_paired_features2(2, 8), deep_supervision=2).to(DEV).train()
    assert ds._native_chain() is not None
    outs = ds(x)
    assert isinstance(outs, list) and [tuple(o.shape) for o in outs] == [(2, 3, 32, 32, 32), (2, 3, 16, 16, 16)]
    y = O.phantom_labels(2, (32, 32, 32), 3).to(DEV)
    L.DeepSupervisionLoss(L.HybirdLoss())(outs, y).backward()
    for p in ds.ds_heads.parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and p.grad.abs().max().item() > 0


def test_plain_unet_graphed_step_equals_eager():
    """Three steps through graph.GraphedTrainStep(warmup=1) - one eager, two replays, Dropout3d on - are the three eager
    steps bit for bit: losses and weights."""
    batches = []
    for i in range(3):
        batches.append((O.synth_image((2, 1, 32, 32, 32), 700 + i).to(DEV), O.phantom_labels(2, (32, 32, 32), 3).to(DEV)))

    def setup():
        torch.manual_seed(16)
        model = network.Unet(1, 3, network.generate_paired_features2(2, 32)).to(DEV)
        network.set_compute_dtype(model, torch.bfloat16)
        model.train()
        ops._drop_counter[0] = 0
        return model, optim.Adam(model.parameters(), lr=1e-3), L.HybirdLoss()

    model_e, opt, crit = setup()
    losses_e = []
    for x, y in batches:
        opt.zero_grad(set_to_none=True)
        loss = crit(model_e(x), y)
        loss.backward()
        opt.step()
        losses_e.append(loss.detach().clone())
    torch.cuda.synchronize()
    losses_e = [float(v) for v in losses_e]
    model_g, opt, crit = setup()
    step = graph.GraphedTrainStep(model_g, crit, opt, warmup=1)
    losses_g = [step(x, y).clone() for x, y in batches]
    torch.cuda.synchronize()
    losses_g = [float(v) for v in losses_g]
    assert step.replays == 2 and step.eager_steps == 1
    assert losses_g == losses_e, (losses_g, losses_e)
    bad = [k for (k, a), (_, b) in zip(model_e.state_dict().items(), model_g.state_dict().items()) if not torch.equal(a, b)]
    assert not bad, bad
    step.release()
