"""The stride-2, transposed and 1x1x1 conv forms below the top level boundary, held to a reference PER KERNEL: every case
calls one op (ops.conv_fwd / conv_dgrad / conv_wgrad / convt_fwd / convt_dgrad / convt_wgrad) inside ops.launch_log()
and first asserts which instantiation the library launched (launch_direct's workgroup-count and tile thresholds,
wgrad_staged_launch's group count, wgrad_reduce_launch's layout test), then compares numbers.  The shapes are the
smallest that land on the kernels a real configuration runs there; both 16-bit builds.

Two comparisons:

  random data    normal operands, weights scaled by 1/sqrt(taps * Cin) (taps * Cin / 8 for ConvTranspose3d); reference =
                 torch CPU fp32 conv on the operands rounded to the storage type; tolerances those of
                 test_mfma_direct_conv_forms_bf16 / test_mfma_convtranspose_bf16 / test_direct_forms_fp16 /
                 test_convtranspose_fp16: forward 2^-8 (bf16) / 2^-11 (fp16) of the reference's maximum + 1e-3, input
                 gradient the same + 2e-3, weight gradient 2e-3 (bf16) / 5e-4 (fp16) of the maximum + 1e-3.
                 Every kernel reached here with a residual (convt_tile_mfma, conv_direct_mfma<.,T>,
                 conv_direct_ksplit<.,T,.>) adds it to the fp32 accumulator and rounds ONCE, so the residual cases use
                 the plain half-ulp term, not the 1.5 x of a stored intermediate.

  integer lattice  the weight gradient once more with x and dy uniform in {-2 .. 2}: every value is exact in bf16 and
                 fp16, every product and every partial sum is an integer of magnitude <= 4 P < 2^24 (P = positions
                 summed), so fp32 accumulation is exact in ANY order and the result cannot depend on the group count,
                 the slab count or the reduce kernel: torch.equal against a float64 reference (27 matrix products; fp32
                 for case A, equally exact under the same premise, which the test asserts).  A dropped position or a
                 misplaced reduce tile, which a tolerance of a fraction of the tensor's maximum can hide, cannot pass.

Run with `-m gpu`.  The transposed conv's wrappers ops.convt_fwd, convt_dgrad and convt_wgrad are the entry points
ru3d_convtranspose3d_k3s2p1_fwd, ru3d_convtranspose3d_k3s2p1_dgrad and ru3d_convtranspose3d_k3s2p1_wgrad."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no HIP device", allow_module_level=True)

import _native as N  # noqa: E402
import _ops as ops  # noqa: E402

DEV = torch.device("cuda:0")
F = torch.nn.functional
DTYPES = [torch.bfloat16, torch.float16]
EPS = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}      # half an ulp relative to the value
WGRAD_RTOL = {torch.bfloat16: 2e-3, torch.float16: 5e-4}
PITCH = 32      # the pitched cases' x is wide[:, 32:] of a buffer this many channels wider

STAGED3, STAGED1 = "wgrad_staged_mfma<27,32>", "wgrad_staged_mfma<1,256>"

# Conv3d cases: cin, cout, k, stride, N, x extents (D, H, W), pitched x, and the names each call must report (None: the
# call is not part of the case).
CONV = {
    # fwd: 25 x 31 x 32 = 24800 outputs = 97 blocks x 4 cout blocks = 388 >= 384, last block 224 of 256 lanes live.
    # dgrad: Cin' = 256 -> the 16-wide tile, t16 * 2 = 416 >= 200 -> 64-cout workgroups.  wgrad: odd Do keeps the LDS-DMA
    # kernel out; 32 tile pairs, G = 32; Cin * Cout >= 16384 -> the tiled reduce in the Conv3d layout.
    "A": dict(cin=128, cout=256, k=3, stride=2, n=1, dims=(49, 61, 63), pitched=True,
              fwd="conv_gather_mfma<2,6>", dgrad="convt_tile_mfma<2,2,4,16>",
              wgrad=[STAGED3, "wgrad_reduce_tiled<true>"]),
    # T = 27 * 48 / 16 = 81 iterations = 13 ring laps + 3: three zero-block fetches in the last lap.  132 blocks x 3.
    # (the input and weight gradients of this width take the generic kernels)
    "B": dict(cin=48, cout=96, k=3, stride=2, n=2, dims=(33, 61, 63), pitched=False,
              fwd="conv_gather_mfma<1,6>", dgrad=None, wgrad=None),
    # 1x1x1 stride 2: 198 blocks x 2.  dgrad: the transposed form with k = 1 (no tile kernel for it).  wgrad: 8 pairs,
    # G = 128, 4 slabs per workgroup = 512 slabs of 8192 outputs -> the 8-lane reduce.
    "E": dict(cin=64, cout=128, k=1, stride=2, n=2, dims=(47, 63, 66), pitched=False,
              fwd="conv_gather_mfma<2,2>", dgrad="conv_direct_mfma<2,T>", wgrad=[STAGED1, "wgrad_reduce<8>"]),
    # T = 48 / 16 = 3 iterations on a ring of 2: one zero-block fetch.  391 blocks x 1.
    "E2": dict(cin=48, cout=32, k=1, stride=1, n=1, dims=(40, 50, 50), pitched=False,
               fwd="conv_gather_mfma<1,2>", dgrad=None, wgrad=None),
    # 8 x 7 x 9 outputs: 4 blocks x 8 -> the K-split kernels.  fwd KS = 16 (108 iterations per wave = 13.5 ring laps, last
    # 32-voxel tile half live); dgrad KS = 32, all 8 parity classes, the odd extents leave classes whose last plane is
    # outside.  wgrad: 128 pairs, G = 8.
    "F": dict(cin=256, cout=512, k=3, stride=2, n=2, dims=(15, 13, 17), pitched=True,
              fwd="conv_direct_ksplit<2,F,8>", dgrad="conv_direct_ksplit<2,T,8>",
              wgrad=[STAGED3, "wgrad_reduce_tiled<true>"]),
}

# ConvTranspose3d(k3, s2, p1) + far zero plane.  Its weight gradient is the stride-2 weight gradient with dy as the
# gathered operand; W[ci][co][tap] is then "[cout'][cin'][tap]" of that view, so the reduce runs in the same layout as a
# Conv3d's (s_i == taps): wgrad_reduce_tiled<false> has no caller among the entry points.
CONVT = {
    # fwd: 405 x 1 workgroups, W = 27 a ragged 32-wide tile.  dgrad: 51 x 2 blocks -> K-split, KS = 4.  wgrad: 8 pairs,
    # G = 128; Cin * Cout = 8192 < 16384 and 864 blocks of outputs -> the 64-lane reduce.
    "C": dict(cin=128, cout=64, n=2, dims=(8, 30, 27), pitched=True,
              fwd="convt_tile_mfma<2,2,2,32>", dgrad="conv_direct_ksplit<2,F,8>", wgrad=[STAGED3, "wgrad_reduce<64>"]),
    # config 4's own level-3 extents: hw = 10 < 12 -> no tile kernel, 250 x 2 blocks -> the direct transposed kernel.
    # dgrad: 32 x 4 -> K-split, KS = 8.  wgrad: 32 pairs, G = 32, tiled reduce.
    "D": dict(cin=256, cout=128, n=2, dims=(20, 20, 10), pitched=False,
              fwd="conv_direct_mfma<2,T>", dgrad="conv_direct_ksplit<2,F,8>",
              wgrad=[STAGED3, "wgrad_reduce_tiled<true>"]),
    "G": dict(cin=512, cout=256, n=2, dims=(5, 7, 9), pitched=False,
              fwd="conv_direct_ksplit<2,T,8>", dgrad="conv_direct_ksplit<2,F,8>",
              wgrad=[STAGED3, "wgrad_reduce_tiled<true>"]),
    "H": dict(cin=128, cout=32, n=2, dims=(8, 30, 27), pitched=False,
              fwd="convt_tile_mfma<1,2,2,32>", dgrad=None, wgrad=None),
}


def _close(a, b, rtol, atol, what):
    a = a.detach().float().cpu()
    b = b.detach().float().cpu()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = (a - b).abs().max().item()
    lim = atol + rtol * max(b.abs().max().item(), 1e-30)
    print("%s: max err %.3e, limit %.3e" % (what, err, lim))
    assert err <= lim, "%s: max err %.3e > %.3e" % (what, err, lim)


def _logged(expect, fn, *args, **kw):
    """run one op inside the launch log; the kernels it reports must be exactly `expect` before any number counts"""
    with ops.launch_log() as log:
        out = fn(*args, **kw)
    expect = [expect] if isinstance(expect, str) else list(expect)
    print("%s -> %s" % (fn.__name__, ";".join(log.names)))
    assert log.names == expect, "%s ran %s, this case is for %s" % (fn.__name__, log.names, expect)
    return out


def _device_x(xw, dt, pitched):
    """the forward operand: the whole buffer, or the channel slice [32:] of it (pitch = C + 32)"""
    t = ops.as_input(xw.to(DEV), dt)
    return t[:, PITCH:] if pitched else t


def _zero_far(t):
    t[:, :, -1] = 0
    t[:, :, :, -1] = 0
    t[..., -1] = 0
    return t


def _lattice(shape, g):
    return torch.randint(-2, 3, shape, generator=g).float()


def _wgrad_ref(gathered, dense, k, stride, dtype):
    """dW[o][i][tap] = sum_{n, p} dense[n, o, p] * gathered[n, i, stride * p + tap - k // 2] as k^3 matrix products in
    `dtype`.  A Conv3d's weight gradient with (x, dy); a ConvTranspose3d(k3, s2, p1)'s with (dy, x), which gives
    [Cin][Cout][3][3][3] directly."""
    pad = k // 2
    gp = F.pad(gathered.to(dtype), (pad,) * 6)
    n, co, do, ho, wo = dense.shape
    ci = gathered.shape[1]
    dm = dense.to(dtype).permute(1, 0, 2, 3, 4).reshape(co, -1)
    out = torch.empty(co, ci, k, k, k, dtype=dtype)
    for kd in range(k):
        for kh in range(k):
            for kw in range(k):
                sl = gp[:, :, kd:kd + stride * (do - 1) + 1:stride, kh:kh + stride * (ho - 1) + 1:stride,
                        kw:kw + stride * (wo - 1) + 1:stride]
                out[:, :, kd, kh, kw] = dm @ sl.permute(0, 2, 3, 4, 1).reshape(-1, ci)
    return out


def _conv_out(size, k, s):
    return (size + 2 * (k // 2) - k) // s + 1


def _conv_shapes(c):
    d, h, w = c["dims"]
    k, s = c["k"], c["stride"]
    xs = (c["n"], c["cin"] + (PITCH if c["pitched"] else 0), d, h, w)
    ys = (c["n"], c["cout"], _conv_out(d, k, s), _conv_out(h, k, s), _conv_out(w, k, s))
    return xs, ys


def _convt_shapes(c):
    d, h, w = c["dims"]
    xs = (c["n"], c["cin"] + (PITCH if c["pitched"] else 0), d, h, w)
    ys = (c["n"], c["cout"], 2 * d, 2 * h, 2 * w)
    return xs, ys


@functools.lru_cache(maxsize=None)
def _conv_lattice(case):
    """lattice operands and the exact weight gradient of a Conv3d case: the same for both storage types"""
    c = CONV[case]
    xs, ys = _conv_shapes(c)
    g = torch.Generator().manual_seed(1000 + sum(xs) + sum(ys))
    xw, gy = _lattice(xs, g), _lattice(ys, g)
    p = ys[0] * ys[2] * ys[3] * ys[4]
    assert 4 * p < 2 ** 24      # the premise: every partial sum is an integer that fp32 holds exactly
    xv = xw[:, PITCH:] if c["pitched"] else xw
    # case A (66 GFLOP): fp32, exact under the premise just asserted; the others in float64
    ref = _wgrad_ref(xv, gy, c["k"], c["stride"], torch.float32 if case == "A" else torch.float64).float()
    return xw, gy, ref


@functools.lru_cache(maxsize=None)
def _convt_lattice(case):
    c = CONVT[case]
    xs, ys = _convt_shapes(c)
    g = torch.Generator().manual_seed(2000 + sum(xs) + sum(ys))
    xw, gy = _lattice(xs, g), _zero_far(_lattice(ys, g))       # contract: dy has zero far planes
    assert 4 * xs[0] * xs[2] * xs[3] * xs[4] < 2 ** 24
    xv = xw[:, PITCH:] if c["pitched"] else xw
    return xw, gy, _wgrad_ref(gy, xv, 3, 2, torch.float64).float()


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", sorted(CONV))
def test_conv_forms_random(case, dt):
    c = CONV[case]
    cin, cout, k, stride, pitched = c["cin"], c["cout"], c["k"], c["stride"], c["pitched"]
    xs, ys = _conv_shapes(c)
    g = torch.Generator().manual_seed(sum(xs) + sum(ys) + k)
    xw = torch.randn(xs, generator=g)
    wt = torch.randn(cout, cin, k, k, k, generator=g) * (1.0 / (k ** 3 * cin) ** 0.5)
    b = torch.randn(cout, generator=g)
    x = _device_x(xw, dt, pitched)
    xv = xw[:, PITCH:] if pitched else xw
    pw = ops.pack_weight(wt.to(DEV), N.ROLE_CONV_FWD, dt, stride)
    y = _logged(c["fwd"], ops.conv_fwd, x, pw, b.to(DEV), cout, k, stride)
    xr = xv.to(dt).float().requires_grad_(True)
    wr = wt.to(dt).float().requires_grad_(True)
    ref = F.conv3d(xr, wr, b, stride=stride, padding=k // 2)
    assert tuple(ref.shape) == ys
    _close(y, ref, EPS[dt], 1e-3, "%s fwd" % case)
    if c["dgrad"] is None:
        return
    gy = torch.randn(ys, generator=g)
    rv = torch.randn(xv.shape, generator=g)
    gyd = ops.as_input(gy.to(DEV), dt)
    res = ops.as_input(rv.to(DEV), dt)
    pwd = ops.pack_weight(wt.to(DEV), N.ROLE_CONV_DGRAD, dt, stride)
    gx = _logged(c["dgrad"], ops.conv_dgrad, gyd, pwd, tuple(xv.shape), k, stride, res=res)
    ref.backward(gy.to(dt).float())
    # the residual joins the fp32 accumulator before the only rounding (see the module docstring): half an ulp
    _close(gx, xr.grad + rv.to(dt).float(), EPS[dt], 2e-3, "%s dgrad+res" % case)
    if k == 1 and stride == 2:
        # no output reads an input voxel with an odd coordinate: it comes back as the residual alone, bit for bit
        # (the whole last W plane, index 65, is such a plane)
        gxc, rc = gx.float().cpu(), rv.to(dt).float()
        for dim in (2, 3, 4):
            odd = torch.arange(1, gxc.shape[dim], 2)
            assert torch.equal(gxc.index_select(dim, odd), rc.index_select(dim, odd)), "odd planes of dim %d" % dim
    gw = _logged(c["wgrad"], ops.conv_wgrad, x, gyd, k, stride)
    _close(gw, wr.grad, WGRAD_RTOL[dt], 1e-3, "%s wgrad" % case)


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", sorted(CONVT))
def test_convtranspose_forms_random(case, dt):
    c = CONVT[case]
    cin, cout, pitched = c["cin"], c["cout"], c["pitched"]
    xs, ys = _convt_shapes(c)
    g = torch.Generator().manual_seed(sum(xs) + sum(ys))
    xw = torch.randn(xs, generator=g)
    wt = torch.randn(cin, cout, 3, 3, 3, generator=g) * (1.0 / (27 * cin / 8) ** 0.5)
    b = torch.randn(cout, generator=g)
    x = _device_x(xw, dt, pitched)
    xv = xw[:, PITCH:] if pitched else xw
    pw = ops.pack_weight(wt.to(DEV), N.ROLE_CONVT_FWD, dt)
    y = _logged(c["fwd"], ops.convt_fwd, x, pw, b.to(DEV), cout)
    xr = xv.to(dt).float().requires_grad_(True)
    wr = wt.to(dt).float().requires_grad_(True)
    ref = F.pad(F.conv_transpose3d(xr, wr, b, stride=2, padding=1), (0, 1, 0, 1, 0, 1))
    assert tuple(ref.shape) == ys
    _close(y, ref, EPS[dt], 1e-3, "%s convT fwd" % case)
    yc = y.float().cpu()
    assert float(yc[:, :, -1].abs().max()) == 0 and float(yc[:, :, :, -1].abs().max()) == 0 \
        and float(yc[..., -1].abs().max()) == 0
    if c["dgrad"] is None:
        return
    gy = _zero_far(torch.randn(ys, generator=g))       # contract: dy has zero far planes
    gyd = ops.as_input(gy.to(DEV), dt)
    pwd = ops.pack_weight(wt.to(DEV), N.ROLE_CONVT_DGRAD, dt)
    gx = _logged(c["dgrad"], ops.convt_dgrad, gyd, pwd, tuple(xv.shape))
    ref.backward(gy.to(dt).float())
    _close(gx, xr.grad, EPS[dt], 2e-3, "%s convT dgrad" % case)
    gw = _logged(c["wgrad"], ops.convt_wgrad, x, gyd)
    _close(gw, wr.grad, WGRAD_RTOL[dt], 1e-3, "%s convT wgrad" % case)


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", [k for k in sorted(CONV) if CONV[k]["wgrad"]])
def test_conv_wgrad_lattice_exact(case, dt):
    c = CONV[case]
    xw, gy, ref = _conv_lattice(case)
    x = _device_x(xw, dt, c["pitched"])
    gyd = ops.as_input(gy.to(DEV), dt)
    gw = _logged(c["wgrad"], ops.conv_wgrad, x, gyd, c["k"], c["stride"]).cpu()
    assert gw.shape == ref.shape
    bad = int((gw != ref).sum())
    print("%s lattice wgrad: %d of %d entries differ" % (case, bad, ref.numel()))
    assert torch.equal(gw, ref), "%d of %d entries differ, first at %s" % (
        bad, ref.numel(), (gw != ref).nonzero()[0].tolist())


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", [k for k in sorted(CONVT) if CONVT[k]["wgrad"]])
def test_convtranspose_wgrad_lattice_exact(case, dt):
    c = CONVT[case]
    xw, gy, ref = _convt_lattice(case)
    x = _device_x(xw, dt, c["pitched"])
    gyd = ops.as_input(gy.to(DEV), dt)
    gw = _logged(c["wgrad"], ops.convt_wgrad, x, gyd).cpu()
    assert gw.shape == ref.shape
    bad = int((gw != ref).sum())
    print("%s lattice convT wgrad: %d of %d entries differ" % (case, bad, ref.numel()))
    assert torch.equal(gw, ref), "%d of %d entries differ, first at %s" % (
        bad, ref.numel(), (gw != ref).nonzero()[0].tolist())


def test_wgrad_reference_matches_torch_on_cpu():
    """The matrix-product reference of the lattice tests against torch's own fp32 ConvTranspose3d backward on case G's
    shape: under the lattice premise fp32 and float64 give the same integers, so all three agree bit for bit."""
    xw, gy, ref = _convt_lattice("G")
    c = CONVT["G"]
    wr = torch.zeros(c["cin"], c["cout"], 3, 3, 3, requires_grad=True)
    F.pad(F.conv_transpose3d(xw, wr, None, stride=2, padding=1), (0, 1, 0, 1, 0, 1)).backward(gy)
    assert torch.equal(wr.grad, ref)
    assert torch.equal(_wgrad_ref(gy, xw, 3, 2, torch.float32), ref)


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
def test_launch_log_does_not_change_results(dt):
    """case C's three ops outside ops.launch_log() and inside it: the same bits"""
    c = CONVT["C"]
    xs, ys = _convt_shapes(c)
    g = torch.Generator().manual_seed(77)
    xw = torch.randn(xs, generator=g)
    wt = torch.randn(c["cin"], c["cout"], 3, 3, 3, generator=g) * (1.0 / (27 * c["cin"] / 8) ** 0.5)
    b = torch.randn(c["cout"], generator=g).to(DEV)
    gyd = ops.as_input(_zero_far(torch.randn(ys, generator=g)).to(DEV), dt)
    x = _device_x(xw, dt, c["pitched"])
    pw = ops.pack_weight(wt.to(DEV), N.ROLE_CONVT_FWD, dt)
    pwd = ops.pack_weight(wt.to(DEV), N.ROLE_CONVT_DGRAD, dt)
    in_shape = (xs[0], c["cin"]) + tuple(xs[2:])
    plain = (ops.convt_fwd(x, pw, b, c["cout"]), ops.convt_dgrad(gyd, pwd, in_shape), ops.convt_wgrad(x, gyd).clone())
    logged = (_logged(c["fwd"], ops.convt_fwd, x, pw, b, c["cout"]),
              _logged(c["dgrad"], ops.convt_dgrad, gyd, pwd, in_shape),
              _logged(c["wgrad"], ops.convt_wgrad, x, gyd))
    for what, p, q in zip(("fwd", "dgrad", "wgrad"), plain, logged):
        assert torch.equal(p, q), what
