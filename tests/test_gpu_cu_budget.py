"""The persistent kernels under the CU budgets a data-parallel run sets (parallel.GradSync: ru3d_set_cu_budget_device(dev,
total - reserve_cus), 240 of 256 by default; RU3D_RESERVE_CUS picks another).  Every conv and weight-gradient family
whose grid - and whose whole work decomposition - comes from ru3d_get_cu_budget() runs here at 240 and at 208, and once
more under a small budget at a shape where the plan hands some workgroups more units than others (units % grid != 0), so
that the unit loop's later trips, the XCD remap, the rings carried from unit to unit and the statistics rows of a
workgroup whose run crosses a sample boundary are executed and compared.  Each case first asserts the launch log exactly
(it must run the family it is named for under that budget), then compares with the CPU reference on operands rounded
to the storage type, at the neighbouring tests' tolerances:

  conv forward / input gradient   EPS[dt] of the reference's maximum + 1e-3, 1.5 EPS[dt] with a residual
                                  (tests/test_gpu_s1_routing.py, tests/test_gpu_pairs.py, tests/test_gpu_inner_boundaries.py)
  fused statistics                mean 1e-5 / 2e-5 and scale 2e-5 / 1e-6 (relative / absolute) against float64 statistics
                                  of the stored y (tests/test_gpu_s1_routing.py); the stride-2 pair form mean 1e-5 and
                                  scale 1e-4 absolute (tests/test_gpu_pairs.py test_s2_pair_fwd_in)
  weight gradients                2e-3 of the gradient's maximum + 1e-3 (tests/test_gpu_wgrad_routing.py)

How units and grids below were derived (csrc/*.hip, B = budget, all divisions integer):

  sliding convs  slide_conv_plan / slide64_conv_plan: cols = N (H / TH) ceil(W / 32) with TH = 8 (slide32) or 4 (slide64),
                 units = cols * dsplit (dsplit | D, D / dsplit a multiple of 4), ny = Cout / 32 (slide32) or max(1, Cout / 64)
                 (slide64), grid = min(units, B / ny), rounded down to a multiple of 8 when units % 8 == 0.  The kernel deals
                 unit ui = blockIdx.x + k grid; with units % 8 == 0 and grid % 8 == 0 it remaps u = (ui % 8)(units / 8) +
                 ui / 8.  D = 4 allows only dsplit = 1.
  pc / pc4       conv3_s1_plan + pc_grid: tiles = N ceil(D/td) ceil(H/th) ceil(W/tw) (pc4: N (D/4)(H/4) ceil(W/32)), gy =
                 Cout / 64 (Cout % 64 == 0) or Cout / 32, gx = (B / gy) rounded down to a multiple of 8 (at least 8, at most
                 tiles).  Workgroup b works on XCD label b % 8: tiles [tiles l / 8, tiles (l + 1) / 8), strided by the
                 workgroups of that label - always several tiles per workgroup.
  conv_ws        conv_ws_slices: one workgroup per (sample, 32 couts, slice); slices = min(B / (N Cout / 32), Cin / 32).  No
                 unit loop: what the budget changes is how the Cin / 32 chunks are cut into slices.
  stride-2 tiles g_plan / t_plan (conv_s2.hip): cols = N ceil(H' / 4) ceil(W' / 16) on the output (conv) or input
                 (transposed) grid, units = cols * dsplit, DL = ceil(D' / dsplit), ny = Cout / 64 (conv) or Cout / 32
                 (transposed), grid as for the sliding convs.
  weight grads   wgrad_slide_plan: pairs = (Cin / 32)(Cout / 32), units = N (H / 8) ceil(W / 32) dsplit (dsplit | D, D / dsplit
                 a multiple of 4, dsplit <= D / 8), G = min(units, B / pairs) workgroups (= slabs) per pair.  wgrad_s2_plan:
                 pairs = (Cin / 32)(Cout / (32 nco)), units = N (Do / 2)(Ho / 2)(Wo / tw), G = min(units, B / pairs).

What the host queries show of a grid: ru3d_conv3d_s2_pair_fwd_in_workspace_bytes is the statistics slab itself (grid * ny *
4 waves * N * 64 channels * 2 floats) and ru3d_conv3d_wgrad_pair_workspace_bytes is G slabs of 27 + 1 taps, so both are
asserted.  ru3d_conv3d_fwd_in_workspace_bytes and the transposed conv's query are floored by the separate statistics
pass's scratch (16 MiB and more at these shapes), which hides the slab; ru3d_conv3d_wgrad_workspace_bytes is the larger of
G slabs and the slabs of the family that would run otherwise (tile kernel: min(512 / pairs, tiles); staged kernel:
min(1024 / pairs, positions / 32)), so it is asserted as that maximum.  Run with `-m gpu`."""
import contextlib
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no HIP device", allow_module_level=True)

import _native as N  # noqa: E402
import _ops as ops  # noqa: E402
import test_gpu_parity as PARITY  # noqa: E402
import test_gpu_s1_routing as S1  # noqa: E402
import test_gpu_wgrad_routing as WG  # noqa: E402

DEV = torch.device("cuda:0")
F = torch.nn.functional
BF, F16 = torch.bfloat16, torch.float16
EPS = S1.EPS
# the budgets of the uneven cases: multiples of 8, at least 32, small enough that a shape of a few GMAC has more units
# than workgroups
SMALL, MID, HALF = 64, 80, 104
GUARD = 4 << 20


@contextlib.contextmanager
def cu_budget(cus):
    """inside: the calling thread's device has `cus` CUs for the persistent kernels; afterwards the device default again,
    whatever happened inside"""
    before = N.lib.ru3d_get_cu_budget()
    try:
        assert N.lib.ru3d_set_cu_budget(cus) == 0
        assert N.lib.ru3d_get_cu_budget() == cus
        yield before
    finally:
        N.lib.ru3d_set_cu_budget(0)
        after = N.lib.ru3d_get_cu_budget()
        assert after == before, "the CU budget reads %d after the block, %d before it" % (after, before)


@pytest.fixture(autouse=True)
def _budget_is_the_device_default():
    """no test of this module leaves a changed budget behind - and none runs on a device that a kernel has faulted"""
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    assert N.lib.ru3d_get_cu_budget() == cus
    yield
    assert N.lib.ru3d_get_cu_budget() == cus
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:       # a sticky HIP error: every later test would only repeat it
        pytest.exit("the device reports an error after this test: %s" % e, returncode=3)


def _stats_close(y, mean, scale, what):
    yd = y.double()
    S1._close(mean, yd.mean(dim=(2, 3, 4)).reshape(-1), 1e-5, 2e-5, what + " mean")
    S1._close(scale, 1.0 / (yd.var(dim=(2, 3, 4), unbiased=False).reshape(-1) + 1e-5).sqrt(), 2e-5, 1e-6, what + " scale")


def _err(a, b):
    return (a.detach().double().cpu() - b.detach().double().cpu()).abs().max().item()


# ------------------------------------------------------------------------------------------------ 1. convs
FIN = "stats_slab_finalize"
# id: (n, cin, cout, extents, form, {budget: names}, (units, grid) of the sliding / stride-2 plan under every budget
# listed or (tiles, gx) of the pc grid under the last one, None where the family has no unit loop).  cin -> cout is the
# module's conv; forms:
#   "fwd" / "res" / "stats" / "dgrad"   3x3x3 stride 1 as in tests/test_gpu_s1_routing.py (dgrad: the kernel sees cout -> cin)
#   "s2" / "s2_pair"                    3x3x3 stride 2: ops.conv_fwd, and ops.conv_s2_pair_fwd_in (statistics + the 1x1x1
#                                       stride-2 conv of the same input as a second output: <stats, y2>)
#   "convt" / "convt_stats"             ConvTranspose3d(k3 s2 p1) + far plane: ops.convt_fwd / ops.convt_fwd_in
# extents are x's.  The 240 / 208 rows are the routing tests' shapes where the plan keeps them in the family under both
# budgets (units == grid there, except pc / pc4: 128 tiles on 120 / 104, 180 on 80 / 64 workgroups); the U_ rows are the
# uneven ones.
CONV = {
    "slide32": (2, 32, 64, (16, 32, 64), "fwd", {240: ["conv3_s1_slide32"], 208: ["conv3_s1_slide32"]}, (64, 64)),
    "slide32_res": (2, 32, 32, (16, 64, 64), "res", {240: ["conv3_s1_slide32<res>"], 208: ["conv3_s1_slide32<res>"]},
                    (128, 128)),
    "slide32_stats": (2, 32, 64, (16, 32, 64), "stats", {240: ["conv3_s1_slide32<stats>", FIN],
                                                         208: ["conv3_s1_slide32<stats>", FIN]}, (64, 64)),
    "slide32_dgrad": (2, 64, 32, (16, 32, 64), "dgrad", {240: ["conv3_s1_slide32"], 208: ["conv3_s1_slide32"]}, (64, 64)),
    # SMALL = 64, 32 -> 64 at 3 x (4, 96, 48): cols = 3 * 12 * 2 = 72, D = 4 -> dsplit 1, units = 72; ny = 2 -> 64 / 2 = 32
    # workgroups (72 % 8 == 0: already a multiple of 8): 8 workgroups run 3 units, 24 run 2.  cost 3 * 7 = 21 <= 1.6 * 9 + 8:
    # the plan keeps the family.  Remapped deal: workgroups with b % 8 == 2 hold u = 18 + b / 8 + 4 k, k = 0, 1, (2): u = 18
    # .. 23 is sample 0, u = 24 .. 26 sample 1 - 4 of them cross the boundary at 24, two more (b % 8 == 5) the one at 48.
    # W = 48: the last column's far half idles
    "U_slide32": (3, 32, 64, (4, 96, 48), "fwd", {SMALL: ["conv3_s1_slide32"]}, (72, 32)),
    "U_slide32_res": (3, 32, 64, (4, 96, 48), "res", {SMALL: ["conv3_s1_slide32<res>"]}, (72, 32)),
    "U_slide32_stats": (3, 32, 64, (4, 96, 48), "stats", {SMALL: ["conv3_s1_slide32<stats>", FIN]}, (72, 32)),
    "U_slide32_dgrad": (3, 64, 32, (4, 96, 48), "dgrad", {SMALL: ["conv3_s1_slide32"]}, (72, 32)),

    "slide64": (2, 64, 64, (16, 32, 64), "fwd", {240: ["conv3_s1_slide64<1>"], 208: ["conv3_s1_slide64<1>"]}, (128, 128)),
    "slide64_cout32_res": (2, 64, 32, (16, 32, 64), "res", {240: ["conv3_s1_slide64<2,res>"],
                                                            208: ["conv3_s1_slide64<2,res>"]}, (128, 128)),
    "slide64_edge_stats": (2, 64, 64, (16, 40, 40), "stats", {240: ["conv3_s1_slide64<1,stats,edge>", FIN],
                                                              208: ["conv3_s1_slide64<1,stats,edge>", FIN]}, (160, 160)),
    "slide64_edge_cout32": (2, 64, 32, (16, 32, 40), "fwd", {240: ["conv3_s1_slide64<2,edge>"],
                                                             208: ["conv3_s1_slide64<2,edge>"]}, (128, 128)),
    "slide64_dgrad": (2, 64, 64, (16, 32, 64), "dgrad", {240: ["conv3_s1_slide64<1>"], 208: ["conv3_s1_slide64<1>"]},
                      (128, 128)),
    # SMALL = 64, 64 -> 32 / 64 at 3 x (4, 96, 40): cols = 3 * 24 * 2 = 144 (W = 40: a light last column of 8), dsplit 1,
    # units = 144, ny = 1 -> 64 workgroups: 16 run 3 units, 48 run 2.  Heavy-first cost 7 + 7 + 6 = 20 <= 1.7 * 9 + 8.  The
    # remapped deal (144 % 8 == 0) puts u = 36 + b / 8 + 8 k on the workgroups with b % 8 == 2: samples change at 48 and 96,
    # so those 8 workgroups (36 .. 43, 44 .. 51, 52 .. 53) and 4 with b % 8 == 5 (90 .. 97, 98 .. 105) cross a boundary
    "U_slide64_c32_edge": (3, 64, 32, (4, 96, 40), "fwd", {SMALL: ["conv3_s1_slide64<2,edge>"]}, (144, 64)),
    "U_slide64_c32_edge_res": (3, 64, 32, (4, 96, 40), "res", {SMALL: ["conv3_s1_slide64<2,res,edge>"]}, (144, 64)),
    "U_slide64_edge": (3, 64, 64, (4, 96, 40), "fwd", {SMALL: ["conv3_s1_slide64<1,edge>"]}, (144, 64)),
    "U_slide64_edge_stats": (3, 64, 64, (4, 96, 40), "stats", {SMALL: ["conv3_s1_slide64<1,stats,edge>", FIN]}, (144, 64)),
    "U_slide64_edge_dgrad": (3, 64, 64, (4, 96, 40), "dgrad", {SMALL: ["conv3_s1_slide64<1,edge>"]}, (144, 64)),

    # pc4: 2 * 8 * 8 * 1 = 128 tiles of 4 x 4 x 32, gy = 2: 240 / 2 = 120, 208 / 2 = 104 workgroups
    "pc4_res": (2, 32, 128, (32, 32, 32), "res", {240: ["conv3_s1_pc4"], 208: ["conv3_s1_pc4"]}, (128, 104)),
    "pc4_stats": (2, 32, 128, (32, 32, 32), "stats", {240: ["conv3_s1_pc4", FIN], 208: ["conv3_s1_pc4", FIN]}, (128, 104)),
    # SMALL = 64: 3 * 2 * 8 * 3 = 144 tiles (2 x 4 x 32 tiles: 288, x 2 cout slices = 576 >= 512, and 144 * 2 * 4 >= 3 * 64: the
    # 512-voxel form), gy = 2 -> gx = 32: label l owns tiles [18 l, 18 l + 18), 4 workgroups each, 4 or 5 tiles a workgroup;
    # samples change at 48 and 96: the workgroups of labels 2 (36 .. 53) and 5 (90 .. 107) cross a boundary
    "U_pc4_res": (3, 32, 128, (8, 32, 96), "res", {SMALL: ["conv3_s1_pc4"]}, (144, 32)),
    "U_pc4_stats": (3, 32, 128, (8, 32, 96), "stats", {SMALL: ["conv3_s1_pc4", FIN]}, (144, 32)),
    # pc<2,8,16,2,1>: 2 * 18 * 5 * 1 = 180 tiles, gy = 3: 240 / 3 = 80 and 208 / 3 = 69 -> 64 workgroups
    "pc_w16_ragged": (2, 32, 96, (36, 36, 16), "res", {240: ["conv3_s1_pc<2,8,16,2,1>"], 208: ["conv3_s1_pc<2,8,16,2,1>"]},
                      (180, 64)),
    "pc_w16_ragged_stats": (2, 32, 96, (36, 36, 16), "stats", {240: ["conv3_s1_pc<2,8,16,2,1>", FIN],
                                                               208: ["conv3_s1_pc<2,8,16,2,1>", FIN]}, (180, 64)),
    # SMALL = 64: 3 * 6 * 10 * 1 = 180 tiles (x 3 slices = 540 >= 512), gy = 3 -> 64 / 3 = 21 -> gx = 16: label l owns tiles
    # [180 l / 8, 180 (l + 1) / 8), two workgroups each, 11 or 12 tiles a workgroup; samples change at 60 and 120: labels 2
    # (45 .. 66) and 5 (112 .. 134) cross
    "U_pc_w16": (3, 32, 96, (12, 80, 16), "res", {SMALL: ["conv3_s1_pc<2,8,16,2,1>"]}, (180, 16)),
    "U_pc_w16_stats": (3, 32, 96, (12, 80, 16), "stats", {SMALL: ["conv3_s1_pc<2,8,16,2,1>", FIN]}, (180, 16)),

    # conv_ws: 4 samples x 8 cout slices = 32 workgroups per slice: 256 / 32 = 8 slices of one chunk each at the full budget,
    # 240 / 32 = 7 (chunks 1 1 1 1 1 1 2) and 208 / 32 = 6 (1 1 2 1 1 2) here: uneven slices, and 7 / 6 partials to sum
    "conv_ws": (4, 256, 256, (10, 10, 5), "fwd", {240: ["conv_ws", "conv_ksplit_reduce"],
                                                  208: ["conv_ws", "conv_ksplit_reduce"]}, None),
    "conv_ws_res": (4, 256, 256, (10, 10, 5), "res", {240: ["conv_ws", "conv_ksplit_reduce"],
                                                      208: ["conv_ws", "conv_ksplit_reduce"]}, None),
    "conv_ws_dgrad": (4, 256, 256, (10, 10, 5), "dgrad", {240: ["conv_ws", "conv_ksplit_reduce"],
                                                          208: ["conv_ws", "conv_ksplit_reduce"]}, None),

    # stride 2, 32 -> 64 at 2 x (16, 32, 128): output 8 x 16 x 64, cols = 2 * 4 * 4 = 32.  256 CUs: dsplit 8 (256 units of one
    # plane).  240 and 208: 256 units would take two rounds (cost 2 * 5), dsplit 4 one (128 units, cost 7): another plan
    # than the full budget's, units == grid == 128
    "s2": (2, 32, 64, (16, 32, 128), "s2", {240: ["conv3_s2_tile"], 208: ["conv3_s2_tile"]}, (128, 128)),
    "s2_pair": (2, 32, 64, (16, 32, 128), "s2_pair", {240: ["conv3_s2_tile", FIN], 208: ["conv3_s2_tile", FIN]}, (128, 128)),
    # SMALL = 64 at 3 x (4, 96, 128): output 2 x 48 x 64, cols = 3 * 12 * 4 = 144; dsplit 1 (cost 3 * 7) beats 2 (5 * 5): 144
    # units on 64 workgroups, 16 of them run 3.  Remapped as for U_slide64: 12 workgroups cross a sample boundary
    "U_s2": (3, 32, 64, (4, 96, 128), "s2", {SMALL: ["conv3_s2_tile"]}, (144, 64)),
    "U_s2_pair": (3, 32, 64, (4, 96, 128), "s2_pair", {SMALL: ["conv3_s2_tile", FIN]}, (144, 64)),

    # transposed, 64 -> 32 at 2 x (16, 32, 32): cols = 2 * 8 * 2 = 32.  256 CUs: dsplit 8.  240 and 208: dsplit 6, DL = 3 - five
    # chunks of three planes and a last one of one - 192 units == grid
    "convt": (2, 64, 32, (16, 32, 32), "convt", {240: ["convt3_s2_tile"], 208: ["convt3_s2_tile"]}, (192, 192)),
    "convt_stats": (2, 64, 32, (16, 32, 32), "convt_stats", {240: ["convt3_s2_tile", FIN], 208: ["convt3_s2_tile", FIN]},
                    (192, 192)),
    # SMALL = 64 at 3 x (2, 32, 96): cols = 3 * 8 * 6 = 144, dsplit 1 (cost 3 * 4) beats 2 (5 * 3): 144 units on 64 workgroups
    "U_convt": (3, 64, 32, (2, 32, 96), "convt", {SMALL: ["convt3_s2_tile"]}, (144, 64)),
    "U_convt_stats": (3, 64, 32, (2, 32, 96), "convt_stats", {SMALL: ["convt3_s2_tile", FIN]}, (144, 64)),
}
CONV_RUNS = [(c, b, dt) for c in CONV for b in CONV[c][5] for dt in (BF, F16)]


def _run_id(r):
    return "%s-b%d%s" % (r[0], r[1], "-fp16" if r[2] == F16 else "")


@functools.lru_cache(maxsize=8)
def _conv_ref(n, cin, cout, dims, kind, dt):
    """operands (fp32 values, not yet rounded) and the torch CPU reference on the rounded ones; never modified.
    kind: "s1" -> (x, w, b, r, gy, conv, conv^T gy), "s2" -> (x, w3, w1, b3, b1, conv3, conv1), "convt" -> (x, w, b, y)"""
    rt = lambda t: t.to(dt).float()     # noqa: E731
    if kind == "s1":
        xv, wt, b, r, gy = S1._operands(n, cin, cout, dims, n + cin + cout + sum(dims))
        return (xv, wt, b, r, gy, F.conv3d(rt(xv), rt(wt), b, padding=1),
                F.conv_transpose3d(rt(gy), rt(wt), None, padding=1))
    g = torch.Generator().manual_seed(n + cin + cout + sum(dims))
    xv = torch.randn((n, cin) + dims, generator=g)
    if kind == "s2":
        w3 = torch.randn(cout, cin, 3, 3, 3, generator=g) * (1.0 / (27 * cin) ** 0.5)
        w1 = torch.randn(cout, cin, 1, 1, 1, generator=g) * (1.0 / cin ** 0.5)
        b3, b1 = torch.randn(cout, generator=g), torch.randn(cout, generator=g)
        return (xv, w3, w1, b3, b1, F.conv3d(rt(xv), rt(w3), b3, stride=2, padding=1), F.conv3d(rt(xv), rt(w1), b1, stride=2))
    wt = torch.randn(cin, cout, 3, 3, 3, generator=g) * (1.0 / (27 * cin / 8) ** 0.5)
    b = torch.randn(cout, generator=g)
    return xv, wt, b, F.pad(F.conv_transpose3d(rt(xv), rt(wt), b, stride=2, padding=1), (0, 1, 0, 1, 0, 1))


def _conv_call(case, dt):
    """-> (call, check): call() runs the case's one op and returns its outputs; check(outputs) compares them"""
    n, cin, cout, dims, form, _, _ = CONV[case]
    d, h, w = dims
    rt = lambda t: t.to(dt).float()     # noqa: E731
    if form in ("fwd", "res", "stats", "dgrad"):
        xv, wt, b, r, gy, want, want_t = _conv_ref(n, cin, cout, dims, "s1", dt)
        if form == "dgrad":
            pw = ops.pack_weight(wt.to(DEV), N.ROLE_CONV_DGRAD, dt, 1)
            gyd = ops.as_input(gy.to(DEV), dt)
            return (lambda: (ops.conv_dgrad(gyd, pw, (n, cin, d, h, w), 3, 1),),
                    lambda out: S1._close(out[0], want_t, EPS[dt], 1e-3, case))
        pw = ops.pack_weight(wt.to(DEV), N.ROLE_CONV_FWD, dt, 1)
        x, bias = ops.as_input(xv.to(DEV), dt), b.to(DEV)
        if form == "fwd":
            return (lambda: (ops.conv_fwd(x, pw, bias, cout, 3, 1),), lambda out: S1._close(out[0], want, EPS[dt], 1e-3, case))
        if form == "res":       # two roundings: the conv's value, then the sum with the residual
            res = ops.as_input(r.to(DEV), dt)
            return (lambda: (ops.conv_fwd(x, pw, bias, cout, 3, 1, res=res),),
                    lambda out: S1._close(out[0], rt(want) + rt(r), 1.5 * EPS[dt], 1e-3, case))

        def check(out):
            S1._close(out[0], want, EPS[dt], 1e-3, case)
            _stats_close(out[0], out[1], out[2], case)
        return lambda: ops.conv_fwd_in(x, pw, bias, cout, 3, 1), check
    if form in ("s2", "s2_pair"):
        xv, w3, w1, b3, b1, want3, want1 = _conv_ref(n, cin, cout, dims, "s2", dt)
        x = ops.as_input(xv.to(DEV), dt)
        pw3 = ops.pack_weight(w3.to(DEV), N.ROLE_CONV_FWD, dt, 2)
        if form == "s2":
            return (lambda: (ops.conv_fwd(x, pw3, b3.to(DEV), cout, 3, 2),),
                    lambda out: S1._close(out[0], want3, EPS[dt], 1e-3, case))
        pw1 = ops.pack_weight(w1.to(DEV), N.ROLE_CONV_FWD, dt, 2)

        def call():
            out = ops.conv_s2_pair_fwd_in(x, pw3, b3.to(DEV), pw1, b1.to(DEV), cout)
            assert out is not None, "no fused kernel for %s" % case
            return out

        def check(out):
            y3, mean, scale, y1 = out
            S1._close(y3, want3, EPS[dt], 1e-3, case + " conv3")
            S1._close(y1, want1, EPS[dt], 1e-3, case + " conv1")
            yd = y3.double().cpu()
            em = _err(mean, yd.mean(dim=(2, 3, 4)).reshape(-1))
            es = _err(scale, 1.0 / (yd.var(dim=(2, 3, 4), unbiased=False).reshape(-1) + 1e-5).sqrt())
            print("%s: mean err %.3e, scale err %.3e" % (case, em, es))
            assert em < 1e-5 and es < 1e-4
        return call, check
    xv, wt, b, want = _conv_ref(n, cin, cout, dims, "convt", dt)
    x = ops.as_input(xv.to(DEV), dt)
    pw = ops.pack_weight(wt.to(DEV), N.ROLE_CONVT_FWD, dt)
    if form == "convt":
        return lambda: (ops.convt_fwd(x, pw, b.to(DEV), cout),), lambda out: S1._close(out[0], want, EPS[dt], 1e-3, case)

    def check(out):
        S1._close(out[0], want, EPS[dt], 1e-3, case)
        _stats_close(out[0], out[1], out[2], case)
    return lambda: ops.convt_fwd_in(x, pw, b.to(DEV), cout), check


def _s2_slab_bytes(n, cin, cout, dims, dt):
    """ru3d_conv3d_s2_pair_fwd_in_workspace_bytes under the current budget: the statistics slab and nothing else"""
    x = N.Tensor(0x10000, n, dims[0], dims[1], dims[2], cin, cin, 0, 0)
    y = N.Tensor(0x10000, n, dims[0] // 2, dims[1] // 2, dims[2] // 2, cout, cout, 0, 0)
    return int(N.lib.ru3d_conv3d_s2_pair_fwd_in_workspace_bytes(ctypes.byref(x), ctypes.byref(y), N.dtype_code(dt)))


@pytest.mark.parametrize("case,budget,dt", CONV_RUNS, ids=[_run_id(r) for r in CONV_RUNS])
def test_conv_under_a_budget(case, budget, dt):
    n, cin, cout, dims, form, names, plan = CONV[case]
    call, check = _conv_call(case, dt)
    with cu_budget(budget):
        with ops.launch_log() as log:
            out = call()
        torch.cuda.synchronize()
        slab = _s2_slab_bytes(n, cin, cout, dims, dt) if form == "s2_pair" else None
    print("ROUTE %s b%d %s %s" % (case, budget, dt, log.names))
    assert log.names == names[budget]
    if slab is not None:        # the query that shows the grid: slab[grid][ny][4][N][64][2]
        assert slab == plan[1] * (cout // 64) * 4 * n * 64 * 2 * 4, (slab, plan)
        assert case[:2] != "U_" or (plan[0] > plan[1] and plan[0] % plan[1])
    check(out)
    if case[:2] == "U_":
        # no split over K in these forms: every output's sum has the same order whatever the decomposition, so the run
        # with the whole chip (one unit per workgroup) gives the same bits
        with ops.launch_log() as log:
            full = call()
        assert log.names == names[budget]
        assert torch.equal(out[0], full[0]), "%s: %d elements differ from the full-budget run" % (
            case, int((out[0] != full[0]).sum()))


# ------------------------------------------------------------------------------------------------ 2. weight gradients
R64, R8 = WG.R64, WG.R8
# id: (form, n, cin, cout, x extents, stride, {budget: names}, {budget: (units, G, other)}).  Forms as in
# tests/test_gpu_wgrad_routing.py: "conv", "pair", "convt" (x has the extents given, dy twice them), "wide".  `other`:
# slabs of the family that would run otherwise (see the module docstring); the plain query reports max(G, other) slabs.
# (2, 64, 64, (32, 32, 64)) and (32, 32, 48), the routing test's sliding shapes, LEAVE the sliding kernel at 240 and 208: 60 /
# 52 workgroups a pair make dsplit 2 the cheapest, and its 32 units x 4 pairs are under the kernel's floor of 192.  The
# shapes here stay: 64 -> 64 is 4 pairs, so B / 4 = 60 / 52 workgroups a pair.
WGRAD = {
    # (16, 48, 64): cols = 2 * 6 * 2 = 24, dsplit 2 -> 48 units (x 4 pairs = 192) <= 52: one unit per workgroup.  tiles 2 * 8 *
    # 12 * 2 = 384 -> other = 512 / 4 = 128
    "slide": ("conv", 2, 64, 64, (16, 48, 64), 1, {240: ["wgrad3_s1_slide", R64], 208: ["wgrad3_s1_slide", R64]},
              {240: (48, 48, 128), 208: (48, 48, 128)}),
    "slide_pair": ("pair", 2, 64, 64, (16, 48, 64), 1, {240: ["wgrad3_s1_slide<pair>", R64, R64],
                                                        208: ["wgrad3_s1_slide<pair>", R64, R64]},
                   {240: (48, 48, 128), 208: (48, 48, 128)}),
    # (8, 72, 72), a light last column of 8: cols = 2 * 9 * 3 = 54, dsplit 1.  240: 54 workgroups.  208: 52, two of them run two
    # units (heavy-first cost 12 + 8 = 20 <= 1.5 * 8.3 + 8) - and G differs from the full budget's 54
    "slide_light": ("conv", 2, 64, 64, (8, 72, 72), 1, {240: ["wgrad3_s1_slide<edge>", R64], 208: ["wgrad3_s1_slide<edge>", R64]},
                    {240: (54, 54, 128), 208: (54, 52, 128)}),
    "slide_light_pair": ("pair", 2, 64, 64, (8, 72, 72), 1, {240: ["wgrad3_s1_slide<edge,pair>", R64, R64],
                                                             208: ["wgrad3_s1_slide<edge,pair>", R64, R64]},
                         {240: (54, 54, 128), 208: (54, 52, 128)}),
    # MID = 80, (16, 48, 40), a light last column of 8: cols = 2 * 6 * 2 = 24, dsplit 2 -> 48 units on 80 / 4 = 20 workgroups
    # a pair (48 at the full budget): 8 run 3 units, 12 run 2, and the light units - the last third of the heavy-first
    # order - fall to the third and second trips.  Heavy-first cost 12 + 12 + 8 = 32 <= 1.5 * 19.2 + 8
    "U_slide_light": ("conv", 2, 64, 64, (16, 48, 40), 1, {MID: ["wgrad3_s1_slide<edge>", R64]}, {MID: (48, 20, 128)}),
    "U_slide_light_pair": ("pair", 2, 64, 64, (16, 48, 40), 1, {MID: ["wgrad3_s1_slide<edge,pair>", R64, R64]},
                           {MID: (48, 20, 128)}),
    # HALF = 104, (8, 64, 96), full columns: cols = 2 * 8 * 3 = 48, dsplit 1 -> 48 units on 104 / 4 = 26 workgroups a pair
    # (cost 2 * 12 = 24 <= 1.5 * 14.8 + 8)
    "U_slide": ("conv", 2, 64, 64, (8, 64, 96), 1, {HALF: ["wgrad3_s1_slide", R64]}, {HALF: (48, 26, 128)}),
    "U_slide_pair": ("pair", 2, 64, 64, (8, 64, 96), 1, {HALF: ["wgrad3_s1_slide<pair>", R64, R64]}, {HALF: (48, 26, 128)}),

    # stride 2, 64 -> 64 (two cout tiles a workgroup: 2 pairs) at (32, 32, 32): output 16^3, units = 2 * 8 * 8 * 1 = 128 on 120 /
    # 104 workgroups a pair (128 at the full budget: there the slab sum is wgrad_reduce<8>, under 128 slabs <64>).  other =
    # min(1024 / 4, 8192 / 32) = 256
    "s2_dma2": ("conv", 2, 64, 64, (32, 32, 32), 2, {240: ["wgrad3_s2_dma<2>", R64], 208: ["wgrad3_s2_dma<2>", R64]},
                {240: (128, 120, 256), 208: (128, 104, 256)}),
    "s2_dma2_pair": ("pair", 2, 64, 64, (32, 32, 32), 2, {240: ["wgrad3_s2_dma<2,pair>", R64, R64],
                                                          208: ["wgrad3_s2_dma<2,pair>", R64, R64]},
                     {240: (128, 120, 256), 208: (128, 104, 256)}),
    # 64 -> 96 (6 pairs) at (16, 16, 32): units = 2 * 4 * 4 * 1 = 32 <= 240 / 6 and 208 / 6.  other = min(1024 / 6, 2048 / 32) = 64.
    # HALF = 104 at (4, 32, 128): units = 1 * 1 * 8 * 4 = 32 on 104 / 6 = 17 workgroups a pair; other = 64 again
    "s2_dma1": ("conv", 2, 64, 96, (16, 16, 32), 2, {240: ["wgrad3_s2_dma<1>", R64], 208: ["wgrad3_s2_dma<1>", R64]},
                {240: (32, 32, 64), 208: (32, 32, 64)}),
    "s2_dma1_pair": ("pair", 2, 64, 96, (16, 16, 32), 2, {240: ["wgrad3_s2_dma<1,pair>", R64, R64],
                                                          208: ["wgrad3_s2_dma<1,pair>", R64, R64]},
                     {240: (32, 32, 64), 208: (32, 32, 64)}),
    "U_s2_dma1": ("conv", 1, 64, 96, (4, 32, 128), 2, {HALF: ["wgrad3_s2_dma<1>", R64]}, {HALF: (32, 17, 64)}),
    "U_s2_dma1_pair": ("pair", 1, 64, 96, (4, 32, 128), 2, {HALF: ["wgrad3_s2_dma<1,pair>", R64, R64]}, {HALF: (32, 17, 64)}),
    # the register-staged kernel (a sample past the DMA kernel's offsets), one pair: units = 16 * 32 * 2 = 1024 on 240 / 208
    # workgroups - 64 / 192 of them run one unit more.  other = min(1024, 131072 / 32) = 1024
    "s2_tile": ("wide", 1, 32, 32, (64, 128, 128), 2, {240: ["wgrad3_s2_tile", R8], 208: ["wgrad3_s2_tile", R8]},
                {240: (1024, 240, 1024), 208: (1024, 208, 1024)}),
    # ConvTranspose3d 64 -> 64, x 16^3, dy 32^3: the stride-2 weight gradient with dy gathered - s2_dma2's decomposition
    "convt_dma": ("convt", 2, 64, 64, (16, 16, 16), 2, {240: ["wgrad3_s2_dma<2>", R64], 208: ["wgrad3_s2_dma<2>", R64]},
                  {240: (128, 120, 256), 208: (128, 104, 256)}),
}
WGRAD_RUNS = [(c, b, dt) for c in WGRAD for b in WGRAD[c][6] for dt in (BF, F16)]


def _wgrad_queries(form, x, dy, stride, dt):
    """(slabs of the plain query, pair form offered, slabs of the pair query) under the current budget"""
    dx, ddy, code = N.desc(x), N.desc(dy), N.dtype_code(dt)
    cin, cout = (dy.shape[1], x.shape[1]) if form == "convt" else (x.shape[1], dy.shape[1])
    slab = cin * cout * 4
    if form == "convt":
        return N.lib.ru3d_convtranspose3d_k3s2p1_wgrad_workspace_bytes(N.ref(dx), N.ref(ddy), code) / (27 * slab), 0, 0
    plain = N.lib.ru3d_conv3d_wgrad_workspace_bytes(N.ref(dx), N.ref(ddy), 3, stride, code) / (27 * slab)
    ok = N.lib.ru3d_conv3d_wgrad_pair_supported(N.ref(dx), N.ref(ddy), N.ref(ddy), stride, code)
    pair = N.lib.ru3d_conv3d_wgrad_pair_workspace_bytes(N.ref(dx), N.ref(ddy), N.ref(ddy), stride, code) / (28 * slab)
    return plain, ok, pair


def _wgrad_operands(form, dt, n, cin, cout, dims, stride):
    xv, g1, g2, ref, ref2, _ = WG._operands("convt" if form == "convt" else "conv", dt, n, cin, cout, dims, 3, stride)
    if form == "wide":
        x = N.new_act(n, WG.WIDE, dims[0], dims[1], dims[2], dt, DEV)[:, :cin]
        x.copy_(xv.to(DEV))
        assert dims[0] * dims[1] * dims[2] * WG.WIDE >= 2 ** 30
    else:
        x = ops.as_input(xv.to(DEV), dt)
    return x, ops.as_input(g1.to(DEV), dt), ops.as_input(g2.to(DEV), dt) if form == "pair" else None, ref, ref2


@pytest.mark.parametrize("case,budget,dt", WGRAD_RUNS, ids=[_run_id(r) for r in WGRAD_RUNS])
def test_wgrad_under_a_budget(case, budget, dt):
    form, n, cin, cout, dims, stride, names, plans = WGRAD[case]
    units, G, other = plans[budget]
    x, dy, dy2, ref, ref2 = _wgrad_operands(form, dt, n, cin, cout, dims, stride)
    _, _, pair_full = _wgrad_queries(form, x, dy, stride, dt)
    dw2 = None
    with cu_budget(budget):
        plain, pair_ok, pair = _wgrad_queries(form, x, dy, stride, dt)
        with ops.launch_log() as log:
            if form == "pair":
                both = ops.conv_wgrad_pair(x, dy, dy2, stride)
                assert both is not None, "no pair form for %s" % case
                dw, dw2 = both
            elif form == "convt":
                dw = ops.convt_wgrad(x, dy)
            else:
                dw = ops.conv_wgrad(x, dy, 3, stride)
        torch.cuda.synchronize()
    print("ROUTE %s b%d %s %s; query %g slabs, pair %d: %g slabs (%g at the full budget)" % (
        case, budget, dt, log.names, plain, pair_ok, pair, pair_full))
    assert log.names == names[budget]
    assert G <= units and plain == max(G, other)
    if case[:2] == "U_":
        assert G < units and units % G
    if form in ("conv", "pair"):        # the sliding and LDS-DMA kernels offer the pair form: its query is G slabs of 28 taps
        assert pair_ok and pair == G
    WG._close(dw, ref, "%s dW" % case)
    if dw2 is not None:
        WG._close(dw2, ref2, "%s dW2" % case)


def test_wgrad_G_differs_from_the_full_budgets():
    """the cases whose slab count under the budget is not the full budget's: part2 sits at another offset and
    wgrad_reduce sums another number of slabs - what test_wgrad_under_a_budget ran for them"""
    moved = []
    for case in ("slide_light_pair", "U_slide_light_pair", "U_slide_pair", "s2_dma2_pair", "U_s2_dma1_pair"):
        form, n, cin, cout, dims, stride, _, plans = WGRAD[case]
        ydims = tuple((s - 1) // stride + 1 for s in dims)
        x = N.Tensor(0x10000, n, dims[0], dims[1], dims[2], cin, cin, 0, 0)
        dy = N.Tensor(0x10000, n, ydims[0], ydims[1], ydims[2], cout, cout, 0, 0)
        q = lambda: N.lib.ru3d_conv3d_wgrad_pair_workspace_bytes(N.ref(x), N.ref(dy), N.ref(dy), stride, N.BF16) // (  # noqa: E731
            28 * cin * cout * 4)
        full = q()
        for budget, (units, G, _) in plans.items():
            with cu_budget(budget):
                assert q() == G
            if G != full:
                moved.append((case, budget, G, full))
    print(moved)
    assert {m[0] for m in moved} == {"slide_light_pair", "U_slide_light_pair", "U_slide_pair", "s2_dma2_pair", "U_s2_dma1_pair"}


@pytest.mark.parametrize("dt", [BF, F16], ids=["bf16", "fp16"])
def test_wgrad_with_a_budget_below_the_pair_count(dt):
    """tests/test_host_wgrad_plan.py test_small_cu_budget's geometry (64 -> 192 = 12 pairs under 8 CUs) at 1 x (8, 32, 128):
    the full budget runs the sliding kernel (16 units, 256 / 12 = 21 workgroups a pair); 8 / 12 = 0 workgroups a pair is not
    that kernel's, the tile kernel computes the gradient (2 x 4 x 32 tiles: 4 * 8 * 4 = 128, min(512 / 12, 128) = 42 slabs)
    and no pair form is offered"""
    n, cin, cout, dims = 1, 64, 192, (8, 32, 128)
    x, dy, _, ref, _ = _wgrad_operands("conv", dt, n, cin, cout, dims, 1)
    with ops.launch_log() as log:
        full = ops.conv_wgrad(x, dy, 3, 1)
    assert log.names == ["wgrad3_s1_slide", R64]
    with cu_budget(8):
        plain, pair_ok, _ = _wgrad_queries("conv", x, dy, 1, dt)
        with ops.launch_log() as log:
            dw = ops.conv_wgrad(x, dy, 3, 1)
        torch.cuda.synchronize()
    print("ROUTE 64 -> 192 under 8 CUs: %s, %g slabs" % (log.names, plain))
    assert log.names == ["wgrad3_s1_mfma<2,4,32>", R64]
    assert plain == 42 and not pair_ok
    WG._close(dw, ref, "dW under 8 CUs")
    WG._close(full, ref, "dW at the full budget")


# ------------------------------------------------------------------------------------------------ 3. scratch contract
class _Guarded:
    """`nbytes` of scratch inside a larger allocation, NaN-filled, with 0xA5 guard words on both sides (the _Scratch of
    tests/test_gpu_conv_contract.py, with a front guard as well): a kernel that takes the scratch for larger than it is
    fails the guard assertion and writes nowhere else"""

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        self.buf = torch.empty(2 * GUARD + self.nbytes, dtype=torch.uint8, device=DEV)
        self.buf.fill_(0xA5)
        self.ws = self.buf[GUARD:GUARD + self.nbytes]
        self.ws.fill_(0xFF)
        assert self.ws.data_ptr() % 16 == 0

    def intact(self):
        return bool((self.buf[:GUARD] == 0xA5).all()) and bool((self.buf[GUARD + self.nbytes:] == 0xA5).all())

    def untouched(self):
        return bool((self.ws == 0xFF).all())


def _raw_wgrad_pair(x, dy, dy2, dw, dw2, scratch, dt):
    dx, ddy, ddy2 = N.desc(x), N.desc(dy), N.desc(dy2)
    with ops.launch_log() as log:
        rc = N.lib.ru3d_conv3d_wgrad_pair(N.ref(dx), N.ref(ddy), N.ref(ddy2), N.ptr(dw), N.ptr(dw2), N.ptr(scratch.ws),
                                          scratch.nbytes, 1, N.dtype_code(dt), N.stream())
    torch.cuda.synchronize()
    return rc, log.names


def test_wgrad_scratch_queried_under_one_budget_and_used_under_another():
    """GradSync.remove() restores the full budget in the middle of a process.  slide_light_pair's shape: 52 slabs of 28 taps
    under 208 CUs, 54 with the whole chip.  The smaller scratch under the full budget is refused before any launch; the
    larger one under 208 is simply enough."""
    form, n, cin, cout, dims, stride, names, plans = WGRAD["slide_light_pair"]
    dt = BF
    x, dy, dy2, ref, ref2 = _wgrad_operands(form, dt, n, cin, cout, dims, stride)
    dx, ddy, code = N.desc(x), N.desc(dy), N.dtype_code(dt)
    query = lambda: int(N.lib.ru3d_conv3d_wgrad_pair_workspace_bytes(N.ref(dx), N.ref(ddy), N.ref(ddy), 1, code))  # noqa: E731
    with cu_budget(208):
        small = query()
    large = query()
    slab = 28 * cin * cout * 4
    assert (small, large) == (52 * slab, 54 * slab)
    dw = torch.full((cout, cin, 3, 3, 3), -7.0, device=DEV)
    dw2 = torch.full((cout, cin, 1, 1, 1), -7.0, device=DEV)
    s = _Guarded(small)
    rc, launched = _raw_wgrad_pair(x, dy, dy2, dw, dw2, s, dt)
    assert s.intact(), "the pair kernel wrote outside a scratch of 52 slabs"
    assert rc != 0 and launched == [] and b"workspace too small" in N.lib.ru3d_last_error()
    assert s.untouched() and bool((dw == -7.0).all()) and bool((dw2 == -7.0).all())
    s = _Guarded(large)
    with cu_budget(208):
        rc, launched = _raw_wgrad_pair(x, dy, dy2, dw, dw2, s, dt)
    assert s.intact()
    assert rc == 0 and launched == names[208]
    WG._close(dw, ref, "dW on the full budget's scratch under 208 CUs")
    WG._close(dw2, ref2, "dW2 on the full budget's scratch under 208 CUs")


def _raw_s2_pair(x, pw3, b3, pw1, b1, y3, y1, mean, scale, scratch, dt):
    dx, d3, d1 = N.desc(x), N.desc(y3), N.desc(y1)
    with ops.launch_log() as log:
        rc = N.lib.ru3d_conv3d_s2_pair_fwd_in(N.ref(dx), N.ptr(pw3), N.ptr(b3), N.ref(d3), N.ptr(pw1), N.ptr(b1), N.ref(d1),
                                              None, N.ptr(mean), N.ptr(scale), N.ptr(scratch.ws), scratch.nbytes,
                                              ctypes.c_float(1e-5), N.dtype_code(dt), N.stream())
    torch.cuda.synchronize()
    return rc, log.names


def test_stats_slab_queried_under_one_budget_and_used_under_another():
    """The stats conv whose query is its slab and nothing else (the stride-1 query is floored by the separate statistics
    pass's scratch and does not move with the budget): s2_pair's shape, 128 workgroups under 208 CUs, 256 with the whole
    chip."""
    n, cin, cout, dims, _, names, _ = CONV["s2_pair"]
    dt = BF
    xv, w3, w1, b3, b1, want3, want1 = _conv_ref(n, cin, cout, dims, "s2", dt)
    x = ops.as_input(xv.to(DEV), dt)
    pw3 = ops.pack_weight(w3.to(DEV), N.ROLE_CONV_FWD, dt, 2)
    pw1 = ops.pack_weight(w1.to(DEV), N.ROLE_CONV_FWD, dt, 2)
    b3d, b1d = b3.to(DEV), b1.to(DEV)
    with cu_budget(208):
        small = _s2_slab_bytes(n, cin, cout, dims, dt)
    large = _s2_slab_bytes(n, cin, cout, dims, dt)
    row = 4 * n * 64 * 2 * 4
    assert (small, large) == (128 * row, 256 * row)
    od, oh, ow = (s // 2 for s in dims)
    y3, y1 = N.new_act(n, cout, od, oh, ow, dt, DEV), N.new_act(n, cout, od, oh, ow, dt, DEV)
    y3.fill_(-7.0)
    y1.fill_(-7.0)
    mean = torch.full((n * cout,), -7.0, device=DEV)
    scale = torch.full((n * cout,), -7.0, device=DEV)
    s = _Guarded(small)
    rc, launched = _raw_s2_pair(x, pw3, b3d, pw1, b1d, y3, y1, mean, scale, s, dt)
    assert s.intact(), "the stride-2 kernel wrote outside a slab of 128 workgroups"
    assert rc != 0 and launched == [] and b"workspace too small" in N.lib.ru3d_last_error()
    assert s.untouched() and bool((y3 == -7.0).all()) and bool((y1 == -7.0).all()) and bool((mean == -7.0).all())
    s = _Guarded(large)
    with cu_budget(208):
        rc, launched = _raw_s2_pair(x, pw3, b3d, pw1, b1d, y3, y1, mean, scale, s, dt)
    assert s.intact()
    assert rc == 0 and launched == names[208]
    S1._close(y3, want3, EPS[dt], 1e-3, "conv3 on the full budget's slab under 208 CUs")
    S1._close(y1, want1, EPS[dt], 1e-3, "conv1 on the full budget's slab under 208 CUs")
    yd = y3.double().cpu()
    assert _err(mean, yd.mean(dim=(2, 3, 4)).reshape(-1)) < 1e-5
    assert _err(scale, 1.0 / (yd.var(dim=(2, 3, 4), unbiased=False).reshape(-1) + 1e-5).sqrt()) < 1e-4


# ------------------------------------------------------------------------------------------------ 4. one whole step
def test_g1_whole_net_bf16_with_240_cus(golden_dir):
    """what a data-parallel rank executes: tests/test_gpu_parity.py's bf16 whole-net comparison - forward, loss and every
    parameter gradient against the same golden file, at that test's tolerances - with 16 CUs left to RCCL"""
    with cu_budget(240):
        PARITY.test_g1_whole_net_bf16(golden_dir)
        torch.cuda.synchronize()
