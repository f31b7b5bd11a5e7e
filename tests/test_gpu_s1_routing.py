"""Which kernel the 3x3x3 stride-1 dispatch runs (csrc/conv_mfma.hip conv3_s1_plan and its consumer): one case per
kernel family and per launch-time fallback, at the smallest shape that reaches it under the default switches.  Every
case first asserts the launch log exactly - the names carry the instantiation - and then compares the result with torch
CPU on operands rounded to the storage type (tests/test_gpu_pc4.py's tolerances).  The expected names were recorded
from the dispatch as it stood before the plan was folded into one function.  Run with `-m gpu`."""
import contextlib
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no HIP device", allow_module_level=True)

import _native as N  # noqa: E402
import _ops as ops  # noqa: E402

DEV = torch.device("cuda:0")
F = torch.nn.functional
EPS = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
DT = torch.bfloat16
DTYPES = [torch.bfloat16, torch.float16]


def both_types(ids):
    """(id, storage type) pairs and their test ids: every id in bf16 under its own name, then in fp16 as <id>-fp16"""
    pairs = [(i, dt) for dt in DTYPES for i in ids]
    return pairs, [i if dt == torch.bfloat16 else i + "-fp16" for i, dt in pairs]


def _rt(t, dt=DT):
    return t.to(dt).float()


def _close(a, b, rtol, atol, what):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = (a - b).abs().max().item()
    lim = atol + rtol * max(b.abs().max().item(), 1e-30)
    assert err <= lim, "%s: max err %.3e > %.3e" % (what, err, lim)


def _operands(n, cin, cout, dims, seed):
    g = torch.Generator().manual_seed(seed)
    d, h, w = dims
    xv = torch.randn(n, cin, d, h, w, generator=g)
    wt = torch.randn(cout, cin, 3, 3, 3, generator=g) * (1.0 / (27 * cin) ** 0.5)
    b = torch.randn(cout, generator=g)
    r = torch.randn(n, cout, d, h, w, generator=g)
    gy = torch.randn(n, cout, d, h, w, generator=g)
    return xv, wt, b, r, gy


def _fwd_raw(x, pw, bias, y, res=None, with_ws=True):
    """ru3d_conv3d_fwd into a caller-made y (any pitch / pointer), with or without the optional scratch"""
    dx, dy = N.desc(x), N.desc(y)
    dr = N.desc(res) if res is not None else None
    ws, wsn = ops._conv_ws(dx, dy, 3, 1, x.dtype, x.device) if with_ws else (None, 0)
    code = N.dtype_code(x.dtype)
    return N.lib.ru3d_conv3d_fwd(N.ref(dx), N.ptr(pw), N.ptr(bias), N.ref(dr), N.ref(dy), 3, 1, code, code, ws, wsn,
                                 N.stream())


@contextlib.contextmanager
def scratch_short_by(nbytes):
    """inside: the wrappers hand ru3d_conv3d_fwd / _dgrad their optional scratch `nbytes` short of what the query asks"""
    def short(dsrc, ddst, k, stride, dtype, device):
        need = N.lib.ru3d_conv3d_workspace_bytes(N.ref(dsrc), N.ref(ddst), k, stride, N.dtype_code(dtype))
        assert need > nbytes, "the case has no scratch to shorten"
        return N.ptr(N.workspace(need, device)), need - nbytes
    real, ops._conv_ws = ops._conv_ws, short
    try:
        yield
    finally:
        ops._conv_ws = real


# id: (n, cin, cout, dims, what, names).  what: "fwd" (bias), "res" (bias + residual), "stats" (ru3d_conv3d_fwd_in),
# "dgrad" (input gradient of the module conv cin -> cout: the kernel sees cout -> cin channels, flipped taps),
# "no_ws" (forward without the optional scratch), "y8" (forward into a y whose pointer is 8- but not 16-byte aligned),
# "short:fwd" / "short:res" / "short:dgrad" (the form named, on a scratch 16 bytes under the query: the plan is a ladder,
# and the launch takes the first kernel whose partials fit - on the deepest level conv_ws wants 8 slices, conv3_s1_sk 4)
CASES = {
    "slide32": (2, 32, 64, (16, 32, 64), "fwd", ["conv3_s1_slide32"]),
    "slide32_res": (2, 32, 32, (16, 64, 64), "res", ["conv3_s1_slide32<res>"]),
    "slide32_stats": (2, 32, 64, (16, 32, 64), "stats", ["conv3_s1_slide32<stats>", "stats_slab_finalize"]),
    "slide32_dgrad": (2, 64, 32, (16, 32, 64), "dgrad", ["conv3_s1_slide32"]),
    "slide32_y8_falls_through": (2, 32, 64, (16, 32, 64), "y8", ["conv3_s1_mfma<2,4,32,2,1>"]),
    "slide64": (2, 64, 64, (16, 32, 64), "fwd", ["conv3_s1_slide64<1>"]),
    "slide64_cout32_res": (2, 64, 32, (16, 32, 64), "res", ["conv3_s1_slide64<2,res>"]),
    "slide64_edge_stats": (2, 64, 64, (16, 40, 40), "stats", ["conv3_s1_slide64<1,stats,edge>", "stats_slab_finalize"]),
    "slide64_edge_cout32": (2, 64, 32, (16, 32, 40), "fwd", ["conv3_s1_slide64<2,edge>"]),
    "slide64_dgrad": (2, 64, 64, (16, 32, 64), "dgrad", ["conv3_s1_slide64<1>"]),
    "slide64_y8_falls_through": (2, 64, 64, (16, 32, 64), "y8", ["conv3_s1_sk<16>"]),
    "slide64_y8_falls_to_pc4": (2, 64, 128, (16, 32, 64), "y8", ["conv3_s1_pc4"]),
    "conv_ws": (2, 256, 256, (10, 10, 5), "fwd", ["conv_ws", "conv_ksplit_reduce"]),
    "conv_ws_res": (2, 256, 256, (10, 10, 5), "res", ["conv_ws", "conv_ksplit_reduce"]),
    "conv_ws_dgrad": (2, 256, 256, (10, 10, 5), "dgrad", ["conv_ws", "conv_ksplit_reduce"]),
    "conv_ws_no_ws": (2, 256, 256, (10, 10, 5), "no_ws", ["conv3_s1_mfma<2,8,8,1,1>"]),
    "conv_ws_short": (2, 256, 256, (10, 10, 5), "short:fwd", ["conv3_s1_sk<8>", "conv_ksplit_reduce"]),
    "conv_ws_short_res": (2, 256, 256, (10, 10, 5), "short:res", ["conv3_s1_sk<8>", "conv_ksplit_reduce"]),
    "conv_ws_short_dgrad": (2, 256, 256, (10, 10, 5), "short:dgrad", ["conv3_s1_sk<8>", "conv_ksplit_reduce"]),
    "sk16": (2, 256, 256, (16, 16, 16), "fwd", ["conv3_s1_sk<16>"]),
    "sk16_dgrad": (2, 256, 256, (16, 16, 16), "dgrad", ["conv3_s1_sk<16>"]),
    "sk8_split": (3, 256, 128, (4, 8, 24), "res", ["conv3_s1_sk<8>", "conv_ksplit_reduce"]),
    "sk8_split_short": (3, 256, 128, (4, 8, 24), "short:res", ["conv3_s1_sk<8>", "conv_ksplit_reduce"]),
    "sk16_split": (2, 256, 256, (8, 8, 32), "fwd", ["conv3_s1_sk<16>", "conv_ksplit_reduce"]),
    "sk16_split_no_ws": (2, 256, 256, (8, 8, 32), "no_ws", ["conv3_s1_mfma<1,4,32,1,1>"]),
    "sk8_split_no_ws": (2, 512, 512, (8, 8, 8), "no_ws", ["conv3_s1_mfma<2,8,8,1,1>"]),
    "pc4_res": (2, 32, 128, (32, 32, 32), "res", ["conv3_s1_pc4"]),
    "pc4_stats": (2, 32, 128, (32, 32, 32), "stats", ["conv3_s1_pc4", "stats_slab_finalize"]),
    "pc4_dgrad": (2, 128, 32, (32, 32, 32), "dgrad", ["conv3_s1_pc4"]),
    "pc_w32_nt2": (2, 32, 128, (18, 32, 64), "fwd", ["conv3_s1_pc<2,4,32,2,2>"]),
    "pc_w16_ragged": (2, 32, 96, (36, 36, 16), "res", ["conv3_s1_pc<2,8,16,2,1>"]),
    "pc_w16_ragged_stats": (2, 32, 96, (36, 36, 16), "stats", ["conv3_s1_pc<2,8,16,2,1>", "stats_slab_finalize"]),
    "pc_w16_dgrad": (2, 96, 32, (36, 36, 16), "dgrad", ["conv3_s1_pc<2,8,16,2,1>"]),
    "pc_w8": (4, 32, 96, (20, 40, 10), "fwd", ["conv3_s1_pc<4,8,8,2,1>"]),
    "tile_mt1": (1, 32, 32, (8, 8, 8), "res", ["conv3_s1_mfma<2,8,8,1,1>"]),
    "tile_mt1_dgrad": (1, 32, 32, (8, 8, 8), "dgrad", ["conv3_s1_mfma<2,8,8,1,1>"]),
    "tile_mt1_then_separate_stats": (1, 32, 32, (8, 8, 8), "stats",
                                     ["conv3_s1_mfma<2,8,8,1,1>", "instnorm_stats", "instnorm_stats_finalize"]),
    "tile_mt2_one_per_cu": (2, 96, 64, (18, 32, 32), "fwd", ["conv3_s1_mfma<2,4,32,2,1>"]),
    "tile_w8_splitk": (1, 64, 64, (8, 8, 8), "fwd", ["conv3_s1_mfma<4,8,8,2,1>", "conv_ksplit_reduce"]),
    "tile_w16_splitk": (1, 96, 32, (8, 8, 16), "fwd", ["conv3_s1_mfma<2,8,16,2,1>", "conv_ksplit_reduce"]),
    "tile_w16_splitk_no_ws": (1, 96, 32, (8, 8, 16), "no_ws", ["conv3_s1_mfma<1,8,16,1,1>"]),
    "tile_w32_splitk": (1, 96, 32, (4, 8, 32), "res", ["conv3_s1_mfma<2,4,32,2,1>", "conv_ksplit_reduce"]),
    "tile_splitk_no_ws": (1, 128, 128, (8, 8, 8), "no_ws", ["conv3_s1_mfma<2,8,8,1,1>"]),
}


ROUTES, ROUTE_IDS = both_types(sorted(CASES))


@pytest.mark.parametrize("case,DT", ROUTES, ids=ROUTE_IDS)
def test_s1_routing(case, DT):
    """the names are the same for both storage types: the fp16 build is a second compilation of the same dispatch"""
    n, cin, cout, dims, what, names = CASES[case]
    d, h, w = dims
    xv, wt, b, r, gy = _operands(n, cin, cout, dims, len(case) + n + cin + cout + sum(dims))
    xr, wr = _rt(xv, DT), _rt(wt, DT)
    scratch = scratch_short_by(16) if what.startswith("short:") else contextlib.nullcontext()
    what = what[6:] if what.startswith("short:") else what
    if what == "dgrad":
        pw = ops.pack_weight(wt.to(DEV), N.ROLE_CONV_DGRAD, DT, 1)
        gyd = ops.as_input(gy.to(DEV), DT)
        with scratch, ops.launch_log() as log:
            got = ops.conv_dgrad(gyd, pw, (n, cin, d, h, w), 3, 1)
        want, tol = F.conv_transpose3d(_rt(gy, DT), wr, None, padding=1), EPS[DT]
    else:
        pw = ops.pack_weight(wt.to(DEV), N.ROLE_CONV_FWD, DT, 1)
        x = ops.as_input(xv.to(DEV), DT)
        bias = b.to(DEV)
        want, tol = F.conv3d(xr, wr, b, padding=1), EPS[DT]
        res = ops.as_input(r.to(DEV), DT) if what == "res" else None
        with scratch, ops.launch_log() as log:
            if what == "fwd":
                got = ops.conv_fwd(x, pw, bias, cout, 3, 1)
            elif what == "res":
                got = ops.conv_fwd(x, pw, bias, cout, 3, 1, res=res)
            elif what == "stats":
                got, mean, scale = ops.conv_fwd_in(x, pw, bias, cout, 3, 1)
            elif what == "no_ws":
                got = N.new_act(n, cout, d, h, w, DT, DEV)
                N.check(_fwd_raw(x, pw, bias, got, with_ws=False), "conv3d_fwd")
            else:   # "y8": channels 4 .. 4 + cout of a wider buffer - pitch a multiple of 8, pointer 8 bytes in
                wide = N.new_act(n, cout + 8, d, h, w, DT, DEV)
                got = wide[:, 4:4 + cout]
                assert got.data_ptr() % 16 == 8
                N.check(_fwd_raw(x, pw, bias, got), "conv3d_fwd")
        if what == "res":       # two roundings: the conv's value, then the sum with the residual
            want, tol = _rt(want, DT) + _rt(r, DT), 1.5 * EPS[DT]
    print("ROUTE %s %s %s" % (case, DT, log.names))
    assert log.names == names
    _close(got, want, tol, 1e-3, case)
    if what == "stats":
        yd = got.double()
        _close(mean, yd.mean(dim=(2, 3, 4)).reshape(-1), 1e-5, 2e-5, "mean")
        _close(scale, 1.0 / (yd.var(dim=(2, 3, 4), unbiased=False).reshape(-1) + 1e-5).sqrt(), 2e-5, 1e-6, "scale")


MISALIGNED = {"slide32": (2, 32, 64, (16, 32, 64)), "slide64": (2, 64, 64, (16, 32, 64))}
REFUSED, REFUSED_IDS = both_types(sorted(MISALIGNED))


@pytest.mark.parametrize("shape,DT", REFUSED, ids=REFUSED_IDS)
def test_misaligned_y_with_statistics_is_refused(shape, DT):
    """the slab was planned for the sliding kernel's grid: with a y that kernel cannot store to, ru3d_conv3d_fwd_in is an
    error (and launches nothing), not a run of another kernel into that slab"""
    n, cin, cout, dims = MISALIGNED[shape]
    d, h, w = dims
    xv, wt, b, _, _ = _operands(n, cin, cout, dims, 5)
    x = ops.as_input(xv.to(DEV), DT)
    pw = ops.pack_weight(wt.to(DEV), N.ROLE_CONV_FWD, DT, 1)
    y = N.new_act(n, cout + 8, d, h, w, DT, DEV)[:, 4:4 + cout]
    mean = torch.empty(n * cout, dtype=torch.float32, device=DEV)
    scale = torch.empty(n * cout, dtype=torch.float32, device=DEV)
    dx, dy = N.desc(x), N.desc(y)
    code = N.dtype_code(DT)
    ws = N.workspace(N.lib.ru3d_conv3d_fwd_in_workspace_bytes(N.ref(dx), N.ref(dy), 3, 1, code), DEV)
    with ops.launch_log() as log:
        rc = N.lib.ru3d_conv3d_fwd_in(N.ref(dx), N.ptr(pw), N.ptr(b.to(DEV)), N.ref(dy), 3, 1, code, None, N.ptr(mean),
                                      N.ptr(scale), N.ptr(ws), ws.numel(), ctypes.c_float(1e-5), N.stream())
    assert rc != 0 and b"fused statistics need y" in N.lib.ru3d_last_error()
    assert log.names == []
