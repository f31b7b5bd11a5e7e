"""ConvDirectPlan (conv.h) tied to what runs: what ru3d_conv3d_plan_names reports for a geometry - the figure
tests/test_host_direct_plan.py pins for a sweep - is what the launch log shows when an op of that geometry runs.

  logged cases    the forward and input-gradient calls of cases A, E, F, C, D, G of test_gpu_inner_boundaries.py (its
                  shapes; the numbers are held to a reference there) and the smallest cubic shapes at two samples whose
                  plan begins with an LDS-DMA tile kernel, found with the host query under 256 CUs: 64 -> 64 channels
                  from 11^3 to 22^3 (convt3_s2_tile; 10^3 has too few units to fill the chip) and 32 -> 64 from 31^3 to
                  16^3 (conv3_s2_tile; 30^3 -> 15^3 likewise).  The first thing each checks is log == first name.
  fallback cases  the two tile shapes once more with an operand only the launch knows to be unfit, so that the plan's
                  SECOND name runs, held to torch CPU fp32 on storage-rounded operands with
                  test_gpu_inner_boundaries.py's tolerances (forward: half an ulp of the maximum + 1e-3, input gradient
                  + 2e-3; conv_direct_ksplit adds the residual to the fp32 accumulator and rounds once).
                  The operand is the RESIDUAL: a channel slice at an 8-byte, not 16-byte, aligned base for the
                  transposed form (the tile kernel stores 16-byte rows), any residual for the gather form (its tile
                  kernel has none).  An x at such a base never reaches the plan: every MFMA conv refuses it
                  (conv_mfma_launch: x, w, bias 16-byte aligned), which test_misaligned_x_is_refused_before_the_plan
                  holds; tests/test_gpu_conv_contract.py has no misaligned case of either kind.
  bit equality    on the same two shapes the fused entry points and the plain ones give the same bits: what a block
                  recomputed under activation checkpointing relies on.

Run with `-m gpu`."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no HIP device", allow_module_level=True)

import _native as N  # noqa: E402
import _ops as ops  # noqa: E402
import test_gpu_inner_boundaries as IB  # noqa: E402

DEV = IB.DEV
F = torch.nn.functional
DTYPES = IB.DTYPES
IDS = ["bf16", "fp16"]
# the smallest tile shapes: samples, (cin, cout) of the Conv3d / ConvTranspose3d-like op, full-resolution extents
T_SHAPE = dict(n=2, c=64, lo=(11, 11, 11), hi=(22, 22, 22))     # 64 channels on both grids
G_SHAPE = dict(n=2, cin=32, cout=64, hi=(31, 31, 31), lo=(16, 16, 16))
T_NAMES = ["convt3_s2_tile", "conv_direct_ksplit<2,T,8>"]
G_NAMES = ["conv3_s2_tile", "conv_direct_ksplit<2,F,8>"]


def plan_names(x, cout, out_dims, k, stride, transposed):
    """ru3d_conv3d_plan_names of the conv that gathers from the device tensor x and writes cout dense channels"""
    dx = ops.desc(x)
    dy = N.Tensor(dx.ptr, x.shape[0], out_dims[0], out_dims[1], out_dims[2], cout, cout, 0, 0)
    buf = ctypes.create_string_buffer(256)
    ops.check(N.lib.ru3d_conv3d_plan_names(ops.ref(dx), ops.ref(dy), k, stride, transposed, N.dtype_code(x.dtype), buf,
                                           len(buf)), "conv3d_plan_names")
    return buf.value.decode().split("|")


def _logged_first(names, fn, *args, **kw):
    """run one op inside the launch log: it must have run the plan's first choice"""
    with ops.launch_log() as log:
        out = fn(*args, **kw)
    print("%s -> %s, plan %s" % (fn.__name__, ";".join(log.names), "|".join(names)))
    assert log.names == names[:1], "%s ran %s, the plan says %s" % (fn.__name__, log.names, names)
    return out


def _rand(shape, dt, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return ops.as_input(torch.randn(shape, generator=g, device=DEV), dt)


def _weight(shape, fan, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * (1.0 / fan ** 0.5)


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", ["A", "E", "F"])
def test_conv_cases_run_the_plans_first_choice(case, dt):
    c = IB.CONV[case]
    cin, cout, k, stride = c["cin"], c["cout"], c["k"], c["stride"]
    xs, ys = IB._conv_shapes(c)
    xw = _rand(xs, dt, 1)
    x = xw[:, IB.PITCH:] if c["pitched"] else xw
    wt = _weight((cout, cin, k, k, k), k ** 3 * cin, 2).to(DEV)
    names = plan_names(x, cout, ys[2:], k, stride, 0)
    _logged_first(names, ops.conv_fwd, x, ops.pack_weight(wt, N.ROLE_CONV_FWD, dt, stride), None, cout, k, stride)
    assert names[0] == c["fwd"]
    gy, res = _rand(ys, dt, 3), _rand(tuple(x.shape), dt, 4)
    names = plan_names(gy, cin, xs[2:], k, stride, 1)
    _logged_first(names, ops.conv_dgrad, gy, ops.pack_weight(wt, N.ROLE_CONV_DGRAD, dt, stride), tuple(x.shape), k, stride,
                  res=res)
    assert names[0] == c["dgrad"]


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", ["C", "D", "G"])
def test_convtranspose_cases_run_the_plans_first_choice(case, dt):
    c = IB.CONVT[case]
    cin, cout = c["cin"], c["cout"]
    xs, ys = IB._convt_shapes(c)
    xw = _rand(xs, dt, 5)
    x = xw[:, IB.PITCH:] if c["pitched"] else xw
    wt = _weight((cin, cout, 3, 3, 3), 27 * cin / 8, 6).to(DEV)
    names = plan_names(x, cout, ys[2:], 3, 2, 1)
    _logged_first(names, ops.convt_fwd, x, ops.pack_weight(wt, N.ROLE_CONVT_FWD, dt), None, cout)
    assert names[0] == c["fwd"]
    gy = ops.as_input(IB._zero_far(torch.randn(ys, generator=torch.Generator().manual_seed(7))).to(DEV), dt)
    names = plan_names(gy, cin, xs[2:], 3, 2, 0)
    _logged_first(names, ops.convt_dgrad, gy, ops.pack_weight(wt, N.ROLE_CONVT_DGRAD, dt), tuple(x.shape))
    assert names[0] == c["dgrad"]


def _t_operands(dt):
    """the T shape as the input gradient of a 64 -> 64 pooling conv: dy on 11^3, dx on 22^3"""
    s = T_SHAPE
    g = torch.Generator().manual_seed(11)
    gy = torch.randn((s["n"], s["c"]) + s["lo"], generator=g)
    w3 = _weight((s["c"], s["c"], 3, 3, 3), 27 * s["c"], 12)
    w1 = _weight((s["c"], s["c"], 1, 1, 1), s["c"], 13)
    rv = torch.randn((s["n"], s["c"] + 8) + s["hi"], generator=g)     # the residual's buffer, 8 channels wider
    return gy, w3, w1, rv


def _g_operands(dt):
    """the G shape as a 32 -> 64 pooling conv: x on 31^3, y on 16^3"""
    s = G_SHAPE
    g = torch.Generator().manual_seed(21)
    xv = torch.randn((s["n"], s["cin"]) + s["hi"], generator=g)
    w3 = _weight((s["cout"], s["cin"], 3, 3, 3), 27 * s["cin"], 22)
    w1 = _weight((s["cout"], s["cin"], 1, 1, 1), s["cin"], 23)
    b3, b1 = torch.randn(s["cout"], generator=g), torch.randn(s["cout"], generator=g)
    rv = torch.randn((s["n"], s["cout"]) + s["lo"], generator=g)
    return xv, w3, w1, b3, b1, rv


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_transposed_tile_shape_first_choice_fallback_and_fused_bits(dt):
    s = T_SHAPE
    gy, w3, w1, rv = _t_operands(dt)
    in_shape = (s["n"], s["c"]) + s["hi"]
    gyd = ops.as_input(gy.to(DEV), dt)
    names = plan_names(gyd, s["c"], s["hi"], 3, 2, 1)
    p3 = ops.pack_weight(w3.to(DEV), N.ROLE_CONV_DGRAD, dt, 2)
    gx = _logged_first(names, ops.conv_dgrad, gyd, p3, in_shape, 3, 2)
    assert names == T_NAMES
    # ConvTranspose3d forward is the same form (with the far planes zeroed)
    wt = _weight((s["c"], s["c"], 3, 3, 3), 27 * s["c"] / 8, 14).to(DEV)
    _logged_first(names, ops.convt_fwd, gyd, ops.pack_weight(wt, N.ROLE_CONVT_FWD, dt), None, s["c"])
    # fused pair with a zero partner: the plain entry point's bits
    p1 = ops.pack_weight(w1.to(DEV), N.ROLE_CONV_DGRAD, dt, 2)
    with ops.launch_log() as log:
        pair = ops.conv_s2_dgrad_pair(gyd, p3, torch.zeros_like(gyd), p1, in_shape)
    assert pair is not None and log.names == names[:1], log.names
    assert torch.equal(pair, gx)
    # a residual whose base is 8-byte, not 16-byte aligned (pitch 72: the plan itself still begins with the tile kernel)
    wide = ops.as_input(rv.to(DEV), dt)
    res = wide[:, 4:4 + s["c"]]
    assert res.data_ptr() % 16 == 8 and ops.desc(res).ld % 8 == 0
    with ops.launch_log() as log:
        gxr = ops.conv_dgrad(gyd, p3, in_shape, 3, 2, res=res)
    assert log.names == names[1:], "ran %s, the plan's second choice is %s" % (log.names, names[1:])
    xr = torch.zeros(in_shape, requires_grad=True)
    F.conv3d(xr, w3.to(dt).float(), None, stride=2, padding=1).backward(gy.to(dt).float())
    IB._close(gxr, xr.grad + rv[:, 4:4 + s["c"]].to(dt).float(), IB.EPS[dt], 2e-3, "T fallback dgrad+res")
    IB._close(gx, xr.grad, IB.EPS[dt], 2e-3, "T tile dgrad")


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_gather_tile_shape_first_choice_fallback_and_fused_bits(dt):
    s = G_SHAPE
    xv, w3, w1, b3, b1, rv = _g_operands(dt)
    x = ops.as_input(xv.to(DEV), dt)
    names = plan_names(x, s["cout"], s["lo"], 3, 2, 0)
    p3 = ops.pack_weight(w3.to(DEV), N.ROLE_CONV_FWD, dt, 2)
    y = _logged_first(names, ops.conv_fwd, x, p3, b3.to(DEV), s["cout"], 3, 2)
    assert names == G_NAMES
    # fused pair: y3 has the plain entry point's bits
    p1 = ops.pack_weight(w1.to(DEV), N.ROLE_CONV_FWD, dt, 2)
    with ops.launch_log() as log:
        out = ops.conv_s2_pair_fwd_in(x, p3, b3.to(DEV), p1, b1.to(DEV), s["cout"])
    assert out is not None and log.names == names[:1] + ["stats_slab_finalize"], log.names
    assert torch.equal(out[0], y)
    # the tile kernel has no residual form: with one the second choice runs
    res = ops.as_input(rv.to(DEV), dt)
    with ops.launch_log() as log:
        yr = ops.conv_fwd(x, p3, b3.to(DEV), s["cout"], 3, 2, res=res)
    assert log.names == names[1:], "ran %s, the plan's second choice is %s" % (log.names, names[1:])
    ref = F.conv3d(xv.to(dt).float(), w3.to(dt).float(), b3, stride=2, padding=1)
    IB._close(yr, ref + rv.to(dt).float(), IB.EPS[dt], 1e-3, "G fallback fwd+res")
    IB._close(y, ref, IB.EPS[dt], 1e-3, "G tile fwd")


def test_misaligned_x_is_refused_before_the_plan():
    """x as a channel slice at an 8-byte, not 16-byte, aligned base: refused on the host by conv_mfma_launch's operand
    check, ahead of any plan and of any launch - no fallback kernel takes it"""
    s = G_SHAPE
    dt = torch.bfloat16
    wide = _rand((s["n"], s["cin"] + 8) + s["hi"], dt, 31)
    x = wide[:, 4:4 + s["cin"]]
    assert x.data_ptr() % 16 == 8
    p3 = ops.pack_weight(_weight((s["cout"], s["cin"], 3, 3, 3), 27 * s["cin"], 32).to(DEV), N.ROLE_CONV_FWD, dt, 2)
    with ops.launch_log() as log:
        with pytest.raises(N.Ru3dError, match="16-byte"):
            ops.conv_fwd(x, p3, None, s["cout"], 3, 2)
    assert log.names == []
