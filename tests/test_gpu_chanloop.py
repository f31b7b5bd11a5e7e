"""The "channel loop" family of csrc/norm.hip held to float64 at the edges of its shared geometry: InstanceNorm statistics,
apply and the three-launch backward (reduce2 mode 3 / 4 -> bwd_finalize -> in_lrelu_bwd_kernel), the BatchNorm twins, the
attention gate's pointwise ops, channel-slice copy / add, the fp32 cast and the layout repack.

Every kernel of the family derives its launch from make_chanloop (G, Gb, vpb, span, chunks) and pick_vec (8, 4, 2 or 1
elements per access from C, every operand's pitch and every operand's pointer alignment).  The cases below are chosen by
that geometry - each vector width, pitched and offset operands, idle tail lanes, two group blocks, fewer voxels than voxel
lanes, the three far-plane branches, the chunk cap - and each case states the width it must select and that it does NOT
take the whole-instance kernels of norm_small.hip (tests/test_gpu_small_norm.py has those).

References are float64 restatements of the reference formulas on the STORED tensors (network.py:384-386, 411-416, the
comments above bn_pool_kernel and pointwise_kernel), so only the kernels' own fp32 arithmetic and output rounding differ.
Operands live in wide NDHWC buffers filled with a NaN bit pattern: a lane read outside the channel slice poisons the
result, a lane written outside it changes the pattern, an output voxel left unwritten stays NaN.  Run with `-m gpu`.  ops.bn_train_stats ends in ru3d_batchnorm_stats_finalize."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no HIP device", allow_module_level=True)

import _native as N  # noqa: E402
import _ops as ops  # noqa: E402
# make_chanloop and the workspace layout restated: what the launches write, maximised over the widths pick_vec may choose
from test_host_norm_ws import chanloop as _chanloop, ws_need as _ws_need  # noqa: E402

DEV = torch.device("cuda:0")
BF16, FP16, FP32 = torch.bfloat16, torch.float16, torch.float32
ALL = [BF16, FP16, FP32]
NAME = {BF16: "bf16", FP16: "fp16", FP32: "f32"}
EPS = {BF16: 2.0 ** -8, FP16: 2.0 ** -11}
INT = {BF16: torch.int16, FP16: torch.int16, FP32: torch.int32}
SENT = {BF16: 0x7FC1, FP16: 0x7E01, FP32: 0x7FC00001}        # quiet NaNs with a payload nothing computes
SLOPE = ops.LRELU_SLOPE
S32 = float(torch.tensor(SLOPE, dtype=torch.float32))       # the slope as the C ABI receives it (a float)
IN_EPS = 1e-5


# --------------------------------------------------------------------------- pitched, offset, guarded operands
class Slab:
    """[N, C, D, H, W] view at channel offset `off` of an NDHWC buffer [N, V, ld] filled with a sentinel."""

    def __init__(self, n, c, dims, lay, dt, src=None):
        ld, off = lay if lay is not None else (c, 0)
        assert 0 <= off and off + c <= ld
        d, h, w = dims
        self.n, self.c, self.dims, self.ld, self.off, self.dt = n, c, dims, ld, off, dt
        self.buf = torch.empty(n, d * h * w, ld, dtype=dt, device=DEV)
        self.buf.view(INT[dt]).fill_(SENT[dt])
        self.t = self.buf[:, :, off:off + c].unflatten(1, dims).permute(0, 4, 1, 2, 3)
        if src is not None:
            self.t.copy_(src.to(dt))

    def desc(self):
        N.note_device(DEV)
        d, h, w = self.dims
        return N.Tensor(self.t.data_ptr(), self.n, d, h, w, self.c, self.ld, 0, 0)

    def f64(self):
        return self.t.detach().cpu().double()

    def guard_ok(self, what):
        iv = self.buf.view(INT[self.dt])
        lo, hi = iv[:, :, :self.off], iv[:, :, self.off + self.c:]
        assert bool((lo == SENT[self.dt]).all()) and bool((hi == SENT[self.dt]).all()), \
            "%s: lanes outside [%d, %d) of pitch %d were written" % (what, self.off, self.off + self.c, self.ld)


def _vec(dt, c, *slabs):
    """pick_vec restated on the test's own operands: the widest access that C, every pitch and every pointer allow"""
    isz = torch.empty(0, dtype=dt).element_size()
    vec = 16 // isz
    while vec > 1:
        if c % vec == 0 and all(s.ld % vec == 0 and s.t.data_ptr() % (vec * isz) == 0 for s in slabs if s is not None):
            break
        vec //= 2
    return vec


def _geom(dt, n, c, dims, vec, max_iters=64):
    V = dims[0] * dims[1] * dims[2]
    g = _chanloop(V, c, vec, max_iters, n)
    print("%s n=%d c=%d dims=%s: vec=%d G=%d Gb=%d vpb=%d span=%d chunks=%d" % ((NAME[dt], n, c, dims, vec) + g))
    return g


def _not_small(dt, c, dims, *slabs):
    """in_small_mode's shape rule restated: True when ru3d_in_lrelu_bwd must take the three launches of norm.hip"""
    V = dims[0] * dims[1] * dims[2]
    pieces = all(s.ld % 8 == 0 and s.t.data_ptr() % 16 == 0 for s in slabs if s is not None)
    return dt == FP32 or V > 8192 or c % 8 != 0 or not pieces


def _close(a, b, rtol, atol, what):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = (a - b).abs().max().item()
    lim = atol + rtol * max(b.abs().max().item(), 1e-30)
    assert err <= lim, "%s: max err %.3e > %.3e" % (what, err, lim)


def _close_out(dt, got, ref, what):
    """one output rounding of the storage type; fp32: the project's own bound (test_norm_kernels_vs_oracle_bf16_and_fp32)"""
    if dt == FP32:
        _close(got, ref, 2e-5, 2e-5, what)
    else:
        _close(got, ref, EPS[dt], 1e-4, what)


def _stats64(y, drop):
    """mean, scale = s / sqrt(s^2 var + eps) per (n, c) of the stored tensor (network.py:384 with Dropout3d folded in)"""
    yd = y.double().cpu()
    n, c = yd.shape[:2]
    m = yd.mean(dim=(2, 3, 4))
    v = yd.var(dim=(2, 3, 4), unbiased=False)
    s = drop.double().cpu().view(n, c) if drop is not None else torch.ones(n, c, dtype=torch.float64)
    return m, s / (s * s * v + IN_EPS).sqrt()


def _gpre(gout, out, dt, prec=torch.float64):
    """g' = gout * lrelu'(out) as stored: one fp32 multiply by the slope, one rounding to the storage type"""
    g, o = gout.to(prec), out.to(prec)
    return torch.where(o > 0, g, (g * S32).float().to(prec)).to(dt).to(prec)


def _far(dy):
    dy[:, :, -1] = 0
    dy[:, :, :, -1] = 0
    dy[..., -1] = 0
    return dy


def _bwd_ref(gout, out, y, mean, scale, dt, resid, zero_far, prec=torch.float64, m12=None):
    """d/dy of out = lrelu(IN(y) (+ res)) on the stored tensors (autograd of network.py:411-416), evaluated in `prec` in the
    kernel's operand order scale * (g' - m1 - xhat * m2).  resid: xhat from y and g' rounded to the storage type (it is
    stored and read back); otherwise xhat recovered from `out`.  -> dy, g', m1, m2"""
    n, c = out.shape[:2]
    o = out.to(prec)
    g = gout.to(prec)
    mu = mean.to(prec).view(n, c, 1, 1, 1)
    sc = scale.to(prec).view(n, c, 1, 1, 1)
    if resid:
        gp = _gpre(gout, out, dt, prec)
        xh = (y.to(prec) - mu) * sc
    else:
        gp = torch.where(o > 0, g, g * S32)
        xh = torch.where(o > 0, o, o / S32)
    if m12 is None:
        m1 = gp.mean(dim=(2, 3, 4), keepdim=True)
        m2 = (gp * xh).mean(dim=(2, 3, 4), keepdim=True)
    else:
        m1, m2 = (m.to(prec).view(n, c, 1, 1, 1) for m in m12)
    dy = sc * (gp - m1 - xh * m2)
    return (_far(dy) if zero_far else dy), gp, m1, m2


def _check_dy(dt, got, ref64, ref32, smax, what):
    """16-bit: the bound of test_in_lrelu_bwd_small.  fp32: 4 x the error of the same formula evaluated in float32 on the
    CPU (the factor covers the other summation order of m1 / m2 and fused multiply-adds).  -> (err, model err)"""
    got = got.detach().double().cpu()
    err = (got - ref64).abs().max().item()
    if dt == FP32:
        model = (ref32.double() - ref64).abs().max().item()
        lim = 4.0 * model
        print("%s: fp32 dy err %.3e, float32 CPU model err %.3e, bound %.3e" % (what, err, model, lim))
        assert err <= lim, "%s: dy err %.3e > 4 x float32 model err %.3e = %.3e" % (what, err, model, lim)
        return err, model
    lim = EPS[dt] * max(ref64.abs().max().item(), 1e-30) + 2e-5 * smax
    assert err <= lim, "%s: dy max err %.3e > %.3e" % (what, err, lim)
    return err, None


def _ws(nbytes):
    return N.workspace(nbytes, DEV)


def _in_bwd(gout, out, y, mean, scale, dy, gpre=None, zero_far=False, gsum=None, dsum=None, ws=None, ws_bytes=None):
    dg, do, dyy, ddy = gout.desc(), out.desc(), y.desc(), dy.desc()
    dp = gpre.desc() if gpre is not None else None
    if ws is None:
        buf = _ws(N.lib.ru3d_reduce_workspace_bytes(N.ref(dyy)))
        ws, ws_bytes = N.ptr(buf), buf.numel()
    return N.lib.ru3d_in_lrelu_bwd(N.ref(dg), N.ref(do), N.ref(dyy), N.ptr(mean), N.ptr(scale), N.ref(ddy), N.ref(dp), ws,
                                   ws_bytes, SLOPE, 1 if zero_far else 0, N.ptr(gsum), N.ptr(dsum), N.dtype_code(y.dt),
                                   N.stream(DEV))


# --------------------------------------------------------------------------- the cases
# The vector-width set of the issue: (C, ld, off) -> elements per access for the 16-bit types and for fp32.  `alt` is a
# second layout of the same width (source and destination of the glue kernels have different pitches).
#            C   (ld, off)   alt (ld, off)  16-bit  fp32
WIDTHS = [(32, (64, 32), (48, 8), 8, 4),
          (32, (44, 4), (52, 12), 4, 4),
          (30, (34, 2), (38, 6), 2, 2),
          (32, (42, 2), (46, 6), 2, 2),
          (15, (17, 1), (19, 3), 1, 1),
          (32, (33, 1), (35, 3), 1, 1)]
WIDTH_IDS = ["c%d_ld%d_off%d" % (c, lay[0], lay[1]) for c, lay, _, _, _ in WIDTHS]

# InstanceNorm / BatchNorm cases: (id, n, C, dims, layout of the inputs, layout of the outputs, 16-bit width, fp32 width,
# dtypes).  None = dense.  Every one stays off norm_small.hip (asserted): V > 8192, C % 8 != 0, a pitch that is no
# multiple of 8, or fp32.
IN_CASES = [
    # levels 0-1 geometry scaled down (bf16: G = 4, vpb = 64), far planes by division (H, W no powers of two), VEC 8
    # through a pitched slice
    ("l0_pitched", 2, 32, (24, 20, 18), (64, 32), (64, 32), 8, 4, ALL),
    ("l1_dense", 1, 64, (21, 20, 20), None, None, 8, 4, ALL),
    # idle tail lanes: bf16 G = 3, vpb = 85, thread 255 idle; VEC 2 G = 15, vpb = 17
    ("tail_g3", 2, 24, (21, 20, 20), None, None, 8, 4, ALL),
    ("tail_g15", 2, 30, (9, 10, 11), (34, 2), (34, 2), 2, 2, ALL),
    # two group blocks, the second nearly empty: G = 260 at VEC 1 through a pitch of 261
    ("two_blocks", 1, 260, (5, 6, 7), (261, 1), (261, 1), 1, 1, ALL),
    # fewer voxels than voxel lanes (dense C = 8 is the small path in the 16-bit types: fp32 there, a pitch of 12 else)
    ("v3_dense", 3, 8, (1, 1, 3), None, None, 8, 4, [FP32]),
    ("v3_ld12", 3, 8, (1, 1, 3), (12, 4), (12, 4), 4, 4, [BF16, FP16]),
    ("v4_ld33", 2, 32, (1, 2, 2), (33, 1), (33, 1), 1, 1, ALL),
    # far planes by masks (H, W powers of two) and with W = 1 (every voxel is far)
    ("far_pow2", 1, 32, (10, 32, 32), None, None, 8, 4, ALL),
    ("far_w1", 1, 16, (12, 1024, 1), (20, 4), (20, 4), 4, 4, ALL),
    # operands of different widths: inputs dense (8 / 4), outputs at pitch 44, offset 4 (4): the minimum must win
    ("mixed", 2, 32, (24, 20, 18), None, (44, 4), 4, 4, ALL),
    # the rest of the width set
    ("w4", 2, 32, (9, 10, 11), (44, 4), (52, 12), 4, 4, ALL),
    ("w2", 2, 32, (9, 10, 11), (42, 2), (46, 6), 2, 2, ALL),
    ("w1_c15", 2, 15, (9, 10, 11), (17, 1), (19, 3), 1, 1, ALL),
    ("w1_c32", 2, 32, (9, 10, 11), (33, 1), (35, 3), 1, 1, ALL),
]
IN_PARAMS = [pytest.param(case, dt, id="%s-%s" % (case[0], NAME[dt])) for case in IN_CASES for dt in case[8]]

_INPUTS = {}


def teardown_module(module):
    """the cached slabs are device memory: release them for the rest of the session"""
    _INPUTS.clear()


def _inputs(case, dt, seed=0):
    """y = 1.5 randn + 0.2, res = 0.5 randn, g = randn (the distributions of test_gpu_small_norm.py) as stored slabs, with
    mean / scale from float64 rounded to float.  Built once per (case, dtype, seed) and never modified."""
    key = (case[0], dt, seed)
    if key not in _INPUTS:
        _, n, c, dims, lin, lout, v16, v32, _ = case
        g = torch.Generator().manual_seed(1000 * seed + n + c + sum(dims))
        shape = (n, c) + dims
        y = Slab(n, c, dims, lin, dt, torch.randn(shape, generator=g) * 1.5 + 0.2)
        res = Slab(n, c, dims, lin, dt, torch.randn(shape, generator=g) * 0.5)
        gout = Slab(n, c, dims, lin, dt, torch.randn(shape, generator=g))
        drop = (torch.rand(n * c, generator=g) > 0.5).float() * 2.0
        drop[0] = 0.0
        drop[-1] = 2.0
        m64, s64 = _stats64(y.t, None)
        mean = m64.float().reshape(-1).to(DEV)
        scale = s64.float().reshape(-1).to(DEV)
        _INPUTS[key] = (y, res, gout, drop.to(DEV), mean, scale, m64, s64)
    return _INPUTS[key]


def _expect_vec(case, dt):
    return case[7] if dt == FP32 else case[6]


# --------------------------------------------------------------------------- 2. InstanceNorm: statistics, apply, backward
@pytest.mark.parametrize("case,dt", IN_PARAMS)
def test_in_stats(case, dt):
    _, n, c, dims, lin, _, _, _, _ = case
    y, _, _, drop, _, _, _, _ = _inputs(case, dt)
    # the statistics read y alone: the width of the INPUT layout ("mixed" has a dense y, 8 / 4, whatever its outputs)
    want = (16 // y.t.element_size()) if case[0] == "mixed" else _expect_vec(case, dt)
    assert _vec(dt, c, y) == want, (_vec(dt, c, y), want, case)
    _geom(dt, n, c, dims, want)
    for dr in (None, drop):
        mean, scale = ops.in_stats(y.t, dr)
        m64, s64 = _stats64(y.t, dr)
        what = "%s drop=%s" % (case[0], dr is not None)
        _close(mean.view(n, c), m64, 0, 2e-6 * max(1.0, m64.abs().max().item()), "mean " + what)
        _close(scale.view(n, c), s64, 2e-6, 1e-7, "scale " + what)
        if dr is not None:
            assert bool((scale[dr == 0] == 0).all()), "a dropped channel must have scale exactly 0"
    y.guard_ok("in_stats input")


@pytest.mark.parametrize("case,dt", IN_PARAMS)
def test_in_lrelu_fwd(case, dt):
    _, n, c, dims, lin, lout, _, _, _ = case
    y, res, _, _, mean, scale, m64, s64 = _inputs(case, dt)
    for r in (None, res):
        out = Slab(n, c, dims, lout, dt)
        vec = _vec(dt, c, y, r, out)
        assert vec == _expect_vec(case, dt), (vec, case)
        _geom(dt, n, c, dims, vec, 16)
        got = ops.in_lrelu_fwd(y.t, mean, scale, res=r.t if r is not None else None, out=out.t)
        assert got.data_ptr() == out.t.data_ptr()
        t = (y.f64() - mean.double().cpu().view(n, c, 1, 1, 1)) * scale.double().cpu().view(n, c, 1, 1, 1)
        if r is not None:
            t = t + r.f64()
        _close_out(dt, out.t, torch.nn.functional.leaky_relu(t, S32), "in_lrelu_fwd %s res=%s" % (case[0], r is not None))
        out.guard_ok("in_lrelu_fwd out")


@pytest.mark.parametrize("case,dt", IN_PARAMS)
def test_in_lrelu_bwd_three_launch(case, dt):
    """ru3d_in_lrelu_bwd where norm.hip's three launches run: plain (mode 3), zero_far, residual (mode 4 + the FROM_GPRE
    apply) with gpre_sum, and residual with dy_sum as well.

    fp32 dy has no bound elsewhere in the project: it is held to 4 x the error of the same formula evaluated in float32
    on the CPU, over seeds 0-2.  The float32 model's own error against float64 is 2.0e-7 .. 2.2e-7 at the (9, 10, 11)
    cases (bound 7.9e-7 .. 8.8e-7); every run prints the kernel's error, the model's and the bound for each case and form."""
    _, n, c, dims, lin, lout, _, _, _ = case
    for seed in ((0, 1, 2) if dt == FP32 else (0,)):
        y, res, gout, _, mean, scale, m64, s64 = _inputs(case, dt, seed)
        smax = float(s64.max())
        for form in ("plain", "zero_far", "resid", "resid_dy_sum"):
            resid = form.startswith("resid")
            zero_far = form == "zero_far"
            out = Slab(n, c, dims, lout, dt)
            ops.in_lrelu_fwd(y.t, mean, scale, res=res.t if resid else None, out=out.t)
            dy = Slab(n, c, dims, lout, dt)
            gpre = Slab(n, c, dims, lout, dt) if resid else None
            yy = y if resid else out
            operands = (gout, out, yy, dy, gpre)
            vec = _vec(dt, c, *operands)
            assert vec == _expect_vec(case, dt), (vec, case)
            assert _not_small(dt, c, dims, *operands), "this case would test norm_small.hip again"
            _geom(dt, n, c, dims, vec)
            gsum = torch.full((c,), float("nan"), dtype=torch.float32, device=DEV) if resid else None
            dsum = torch.full((c,), float("nan"), dtype=torch.float32, device=DEV) if form == "resid_dy_sum" else None
            rc = _in_bwd(gout, out, yy, mean, scale, dy, gpre, zero_far, gsum, dsum)
            N.check(rc, "in_lrelu_bwd")
            what = "%s %s %s seed %d" % (case[0], NAME[dt], form, seed)
            args = (gout.t.cpu(), out.t.cpu(), y.t.cpu(), mean.cpu(), scale.cpu(), dt, resid, zero_far)
            ref, ref_gp, _, _ = _bwd_ref(*args)
            ref32 = _bwd_ref(*args, prec=torch.float32)[0] if dt == FP32 else None
            _check_dy(dt, dy.t, ref, ref32, smax, what)
            if zero_far:
                got = dy.t.cpu()
                far = torch.cat((got[:, :, -1].reshape(-1), got[:, :, :, -1].reshape(-1), got[..., -1].reshape(-1)))
                assert bool((far == 0).all()), "%s: far planes must be exactly 0" % what
            if resid:
                assert torch.equal(gpre.f64(), ref_gp), "%s: stored pre-activation gradient" % what
                _close(gsum, ref_gp.sum(dim=(0, 2, 3, 4)), 1e-5, 1e-4, "%s: gpre_sum" % what)
                gpre.guard_ok(what + " gpre")
            if dsum is not None:
                st = dy.f64()
                e = (dsum.double().cpu() - st.sum(dim=(0, 2, 3, 4))).abs()
                mag = st.abs().sum(dim=(0, 2, 3, 4))
                assert bool((e <= 2e-6 * mag + 1e-6).all()), "%s: dy_sum %.3e" % (what, float((e / (mag + 1e-30)).max()))
            for s in (dy, out, gout, yy):
                s.guard_ok(what)


@pytest.mark.parametrize("case,dt", IN_PARAMS)
def test_in_lrelu_bwd_apply(case, dt):
    """The apply pass alone with the two means given (the half ru3d_conv3d_dgrad_in_bwd uses): m12 from float64."""
    _, n, c, dims, lin, lout, _, _, _ = case
    y, _, gout, _, mean, scale, m64, s64 = _inputs(case, dt)
    out = Slab(n, c, dims, lin, dt)
    ops.in_lrelu_fwd(y.t, mean, scale, out=out.t)
    args = (gout.t.cpu(), out.t.cpu(), None, mean.cpu(), scale.cpu(), dt, False)
    _, _, m1, m2 = _bwd_ref(*args, False)
    m12f = (m1.float().reshape(-1), m2.float().reshape(-1))
    m12 = torch.stack(m12f, dim=1).contiguous().to(DEV)          # [n * c][2]
    for zero_far in (False, True):
        dy = Slab(n, c, dims, lout, dt)
        vec = _vec(dt, c, gout, out, dy)
        assert vec == _expect_vec(case, dt), (vec, case)
        _geom(dt, n, c, dims, vec, 16)
        dg, do, ddy = gout.desc(), out.desc(), dy.desc()
        N.check(N.lib.ru3d_in_lrelu_bwd_apply(N.ref(dg), N.ref(do), N.ptr(mean), N.ptr(scale), N.ptr(m12), N.ref(ddy), SLOPE,
                                              1 if zero_far else 0, N.dtype_code(dt), N.stream(DEV)), "in_lrelu_bwd_apply")
        ref = _bwd_ref(*args, zero_far, m12=m12f)[0]
        ref32 = _bwd_ref(*args, zero_far, prec=torch.float32, m12=m12f)[0] if dt == FP32 else None
        _check_dy(dt, dy.t, ref, ref32, float(s64.max()), "apply %s %s zero_far=%s" % (case[0], NAME[dt], zero_far))
        dy.guard_ok("in_lrelu_bwd_apply dy")


# --------------------------------------------------------------------------- 3. workspace bound
GUARD = 64 << 10


class GuardedWs:
    """exactly `nbytes` of workspace, 256-byte aligned, cut out of the middle of a larger buffer with 64 KB of sentinel on
    each side"""

    def __init__(self, nbytes):
        self.buf = torch.full((nbytes + 2 * GUARD + 256,), 0xA5, dtype=torch.uint8, device=DEV)
        self.lo = GUARD + (-(self.buf.data_ptr() + GUARD)) % 256
        self.nbytes = nbytes
        self.ptr = ctypes.c_void_p(self.buf.data_ptr() + self.lo)
        assert (self.buf.data_ptr() + self.lo) % 256 == 0 and self.lo >= GUARD

    def guard_ok(self, what):
        hi = self.lo + self.nbytes
        assert bool((self.buf[:self.lo] == 0xA5).all()), "%s wrote in front of its workspace" % what
        assert bool((self.buf[hi:] == 0xA5).all()), "%s wrote behind its %d bytes of workspace" % (what, self.nbytes)


# Few voxels, where chunks equals the bound of reduce_ws_bytes and only its + 512 covers the rounding of m12 to 256 bytes.
# V = 1 and 2 run in the 16-bit types only: there y^2 is exact in a float, so the kernel's statistics are exact sums and
# scale keeps its 2e-6 bound even where a channel's voxels coincide (V = 1: var = 0; V = 2: var = ((a - b) / 2)^2 falls to
# 2e-7 among 640 channels, far below eps).  An fp32 y^2 rounded to float moves var by ~1e-7, a large share of var + eps in
# such a channel (a float32 CPU restatement of the sums misses the scale bound 70-fold at C = 320, V = 2): the
# |mean| >> std conditioning of the statistics, which is not this module's question.  fp32 runs from V = 3 on.
WS_CASES = [(2, c, (1, 1, v), dt) for c in (8, 320) for v in (1, 2, 3, 5) for dt in ALL if not (v < 3 and dt == FP32)] + \
    [(2, 512, (8, 8, 8), FP32)]


@pytest.mark.parametrize("n,c,dims,dt", WS_CASES, ids=lambda v: NAME.get(v, str(v)).replace(" ", ""))
def test_workspace_exact(n, c, dims, dt):
    """ru3d_instnorm_stats, ru3d_channel_sum and ru3d_in_lrelu_bwd with dy_sum on exactly ru3d_reduce_workspace_bytes:
    results within their bounds, the bytes on both sides untouched, and that size no smaller than what make_chanloop's
    geometry writes.  One byte less is refused before anything is launched.  The operands sit at pitch C + 4, offset 4
    (reduce_ws_bytes depends on n, C and V alone), so that the backward of the 16-bit cases stays on norm.hip's three
    launches and their three workspace regions: partials, m12, dy-sum partials."""
    g = torch.Generator().manual_seed(n + c + sum(dims))
    shape = (n, c) + dims
    V = dims[0] * dims[1] * dims[2]
    lay = (c + 4, 4)
    y = Slab(n, c, dims, lay, dt, torch.randn(shape, generator=g) * 1.5 + 0.2)
    gout = Slab(n, c, dims, lay, dt, torch.randn(shape, generator=g))
    out = Slab(n, c, dims, lay, dt)
    dy = Slab(n, c, dims, lay, dt)
    assert _vec(dt, c, y, gout, out, dy) == 4
    assert _not_small(dt, c, dims, gout, out, dy), "the backward of this case would run in norm_small.hip, without a workspace"
    dyy = y.desc()
    nbytes = N.lib.ru3d_reduce_workspace_bytes(N.ref(dyy))
    need = _ws_need(n, c, V, y.t.element_size())
    _geom(dt, n, c, dims, 4)
    assert nbytes >= need, "reduce workspace of %d bytes, the launches write %d" % (nbytes, need)
    ws = GuardedWs(nbytes)
    code = N.dtype_code(dt)
    mean = torch.empty(n * c, dtype=torch.float32, device=DEV)
    scale = torch.empty(n * c, dtype=torch.float32, device=DEV)
    N.check(N.lib.ru3d_instnorm_stats(N.ref(dyy), None, N.ptr(mean), N.ptr(scale), ws.ptr, nbytes, IN_EPS, code,
                                      N.stream(DEV)), "instnorm_stats")
    m64, s64 = _stats64(y.t, None)
    _close(mean.view(n, c), m64, 0, 2e-6 * max(1.0, m64.abs().max().item()), "mean")
    _close(scale.view(n, c), s64, 2e-6, 1e-7, "scale")
    ws.guard_ok("instnorm_stats")
    csum = torch.empty(c, dtype=torch.float32, device=DEV)
    N.check(N.lib.ru3d_channel_sum(N.ref(dyy), N.ptr(csum), ws.ptr, nbytes, code, N.stream(DEV)), "channel_sum")
    yd = y.f64()
    e = (csum.double().cpu() - yd.sum(dim=(0, 2, 3, 4))).abs()
    assert bool((e <= 2e-6 * yd.abs().sum(dim=(0, 2, 3, 4)) + 1e-6).all()), "channel_sum %.3e" % float(e.max())
    ws.guard_ok("channel_sum")
    # backward with dy_sum: the plain form (xhat from out)
    ops.in_lrelu_fwd(y.t, mean, scale, out=out.t)
    dsum = torch.full((c,), float("nan"), dtype=torch.float32, device=DEV)
    N.check(_in_bwd(gout, out, out, mean, scale, dy, None, False, None, dsum, ws.ptr, nbytes), "in_lrelu_bwd")
    args = (gout.t.cpu(), out.t.cpu(), None, mean.cpu(), scale.cpu(), dt, False, False)
    ref32 = _bwd_ref(*args, prec=torch.float32)[0] if dt == FP32 else None
    _check_dy(dt, dy.t, _bwd_ref(*args)[0], ref32, float(scale.max()), "in_lrelu_bwd on the exact workspace")
    st = dy.f64()
    e = (dsum.double().cpu() - st.sum(dim=(0, 2, 3, 4))).abs()
    assert bool((e <= 2e-6 * st.abs().sum(dim=(0, 2, 3, 4)) + 1e-6).all()), "dy_sum %.3e" % float(e.max())
    ws.guard_ok("in_lrelu_bwd")
    for sl in (y, gout, out, dy):
        sl.guard_ok("workspace case operands")
    # an argument check: nothing is launched
    for rc in (N.lib.ru3d_instnorm_stats(N.ref(dyy), None, N.ptr(mean), N.ptr(scale), ws.ptr, nbytes - 1, IN_EPS, code,
                                         N.stream(DEV)),
               N.lib.ru3d_channel_sum(N.ref(dyy), N.ptr(csum), ws.ptr, nbytes - 1, code, N.stream(DEV)),
               _in_bwd(gout, out, out, mean, scale, dy, None, False, None, dsum, ws.ptr, nbytes - 1)):
        assert rc < 0 and b"workspace too small" in N.lib.ru3d_last_error(), (rc, N.lib.ru3d_last_error())


def test_chunk_cap_respan():
    """make_chanloop's `chunks > 4096` branch: fp32 (1, 257, (66, 64, 64)) has G = 257 at VEC 1 (two group blocks),
    vpb = 1, span = 64 -> 4224 chunks before the cap, re-spanned to 66 voxels x 4096 chunks.  Statistics and channel sums
    on exactly the reduce workspace.  (278 MB; one case, fp32 only.)"""
    n, c, dims = 1, 257, (66, 64, 64)
    V = 66 * 64 * 64
    y = N.new_act(n, c, *dims, FP32, DEV)
    g = torch.Generator(device=DEV).manual_seed(257)
    y.normal_(0.2, 1.5, generator=g)
    assert _chanloop(V, c, 1, 64, n) == (257, 256, 1, 66, 4096) and -(-V // 64) == 4224
    dyy = N.desc(y)
    nbytes = N.lib.ru3d_reduce_workspace_bytes(N.ref(dyy))
    assert nbytes >= _ws_need(n, c, V, 4)
    ws = GuardedWs(nbytes)
    mean = torch.empty(c, dtype=torch.float32, device=DEV)
    scale = torch.empty(c, dtype=torch.float32, device=DEV)
    csum = torch.empty(c, dtype=torch.float32, device=DEV)
    N.check(N.lib.ru3d_instnorm_stats(N.ref(dyy), None, N.ptr(mean), N.ptr(scale), ws.ptr, nbytes, IN_EPS, N.F32,
                                      N.stream(DEV)), "instnorm_stats")
    N.check(N.lib.ru3d_channel_sum(N.ref(dyy), N.ptr(csum), ws.ptr, nbytes, N.F32, N.stream(DEV)), "channel_sum")
    ws.guard_ok("instnorm_stats / channel_sum")
    yd = y.cpu().permute(0, 2, 3, 4, 1).reshape(V, c).double()      # memory order: no copy besides the widening
    m64 = yd.mean(dim=0)
    v64 = yd.var(dim=0, unbiased=False)
    _close(mean, m64, 0, 2e-6 * max(1.0, m64.abs().max().item()), "mean")
    _close(scale, 1.0 / (v64 + IN_EPS).sqrt(), 2e-6, 1e-7, "scale")
    e = (csum.double().cpu() - m64 * V).abs()
    assert bool((e <= 2e-6 * yd.abs().sum(dim=0) + 1e-6).all()), "channel_sum %.3e" % float(e.max())


# --------------------------------------------------------------------------- 4. BatchNorm twins
BN_CASES = [("bn_g3", 3, 24, (21, 20, 20), None, 8, 4), ("bn_g15", 2, 30, (9, 10, 11), (34, 2), 2, 2),
            ("bn_l0", 2, 32, (24, 20, 18), (64, 32), 8, 4)]


@pytest.mark.parametrize("dt", [BF16, FP32], ids=["bf16", "f32"])
@pytest.mark.parametrize("pad", [0, 3], ids=["full", "padded"])
@pytest.mark.parametrize("with_drop", [False, True], ids=["nodrop", "drop"])
@pytest.mark.parametrize("case", BN_CASES, ids=[b[0] for b in BN_CASES])
def test_batchnorm_twins(case, with_drop, pad, dt):
    """bn_train_stats (reduce2 mode 0 pooled), affine_lrelu_fwd and bn_lrelu_bwd (mode 5 pooled, the AFFINE apply) against
    the float64 formulas in the comment above bn_pool_kernel; c_real < C leaves pad lanes with gamma = 1, beta = 0."""
    _, n, c, dims, lay, v16, v32 = case
    c_real = c - pad
    g = torch.Generator().manual_seed(n + c + sum(dims) + pad + int(with_drop))
    shape = (n, c) + dims
    V = dims[0] * dims[1] * dims[2]
    y = Slab(n, c, dims, lay, dt, torch.randn(shape, generator=g) * 1.5 + 0.2)
    res = Slab(n, c, dims, lay, dt, torch.randn(shape, generator=g) * 0.5)
    gout = Slab(n, c, dims, lay, dt, torch.randn(shape, generator=g))
    drop = (torch.rand(n * c, generator=g) > 0.5).float() * 2.0
    drop[0], drop[-1] = 0.0, 2.0
    drop = drop.to(DEV) if with_drop else None
    norm = torch.nn.BatchNorm3d(c_real).to(DEV)
    with torch.no_grad():
        norm.weight.copy_(torch.rand(c_real, generator=g) + 0.5)
        norm.bias.copy_(torch.randn(c_real, generator=g) * 0.3)
        norm.running_mean.copy_(torch.randn(c_real, generator=g) * 0.1)
        norm.running_var.copy_(torch.rand(c_real, generator=g) + 0.5)
    rm0, rv0 = norm.running_mean.double().cpu(), norm.running_var.double().cpu()
    vec = _vec(dt, c, y)
    assert vec == (v32 if dt == FP32 else v16)
    _geom(dt, n, c, dims, vec)
    fscale, fshift, a, b, count = ops.bn_train_stats(y.t, drop, norm, c_real)
    assert count == n * V
    # float64 on the stored tensor
    yd = y.f64()
    d = drop.double().cpu().view(n, c) if with_drop else torch.ones(n, c, dtype=torch.float64)
    s1 = (d * yd.sum(dim=(2, 3, 4))).sum(dim=0)
    s2 = (d * d * (yd * yd).sum(dim=(2, 3, 4))).sum(dim=0)
    mu = s1 / count
    var = (s2 / count - mu * mu).clamp_min(0.0)
    r = 1.0 / (var + float(norm.eps)).sqrt()
    gam = torch.ones(c, dtype=torch.float64)
    bet = torch.zeros(c, dtype=torch.float64)
    gam[:c_real] = norm.weight.detach().double().cpu()
    bet[:c_real] = norm.bias.detach().double().cpu()
    a64, b64 = d * r, (-mu * r).expand(n, c)
    mean_tol = lambda t: 2e-6 * max(1.0, t.abs().max().item())   # noqa: E731
    _close(a.view(n, c), a64, 2e-6, 1e-7, "a")
    _close(fscale.view(n, c), gam * a64, 2e-6, 1e-7, "fscale")
    _close(b.view(n, c), b64, 0, mean_tol(b64), "b")
    _close(fshift.view(n, c), bet + gam * b64, 0, mean_tol(bet + gam * b64), "fshift")
    if with_drop:
        assert bool((a[drop == 0] == 0).all()) and bool((fscale[drop == 0] == 0).all())
    rm1 = 0.9 * rm0 + 0.1 * mu[:c_real]
    rv1 = 0.9 * rv0 + 0.1 * var[:c_real] * count / (count - 1.0)
    _close(norm.running_mean, rm1, 0, mean_tol(rm1), "running mean")
    _close(norm.running_var, rv1, 0, mean_tol(rv1), "running variance")
    # forward: the AFFINE apply on the stored (fscale, fshift)
    fs = fscale.double().cpu().view(n, c, 1, 1, 1)
    fh = fshift.double().cpu().view(n, c, 1, 1, 1)
    out = Slab(n, c, dims, lay, dt)
    ops.affine_lrelu_fwd(y.t, fscale, fshift, res=res.t, out=out.t)
    _close_out(dt, out.t, torch.nn.functional.leaky_relu(yd * fs + fh + res.f64(), S32), "affine_lrelu_fwd")
    out.guard_ok("affine_lrelu_fwd out")
    # backward on the stored (a, b, fscale)
    dy, gpre, dgamma, dbeta = ops.bn_lrelu_bwd(gout.t, out.t, y.t, a, b, fscale, count, zero_far=True)

    def ref(prec):
        av = a.cpu().to(prec).view(n, c, 1, 1, 1)
        bv = b.cpu().to(prec).view(n, c, 1, 1, 1)
        gp = _gpre(gout.t.cpu(), out.t.cpu(), dt, prec)
        xh = y.t.cpu().to(prec) * av + bv
        t1 = gp.sum(dim=(0, 2, 3, 4), keepdim=True)
        t2 = (gp * xh).sum(dim=(0, 2, 3, 4), keepdim=True)
        dyr = fscale.cpu().to(prec).view(n, c, 1, 1, 1) * (gp - t1 / count - xh * (t2 / count))
        return _far(dyr), gp, t1.reshape(-1), t2.reshape(-1)

    ref_dy, ref_gp, dbeta64, dgamma64 = ref(torch.float64)
    ref32 = ref(torch.float32)[0] if dt == FP32 else None
    _check_dy(dt, dy, ref_dy, ref32, float(fscale.abs().max()), "bn dy %s" % case[0])
    assert torch.equal(gpre.double().cpu(), ref_gp), "stored pre-activation gradient"
    _close(dbeta, dbeta64, 1e-5, 1e-4, "dbeta")
    _close(dgamma, dgamma64, 1e-5, 1e-4, "dgamma")
    for s in (y, res, gout, out):
        s.guard_ok("batchnorm operands")


# --------------------------------------------------------------------------- 5. glue kernels
GLUE_DIMS = [(2, (9, 10, 11)), (1, (1, 1, 3))]
GLUE_IDS = ["v990", "v3"]


def _width_case(width, dt, n, dims, g, k):
    """k random operands at the case's layout / alt layout alternately, and the expected width"""
    c, lay, alt, v16, v32 = width
    return c, [Slab(n, c, dims, (lay, alt)[i % 2], dt, torch.randn((n, c) + dims, generator=g)) for i in range(k)], \
        (v32 if dt == FP32 else v16)


@pytest.mark.parametrize("dt", ALL, ids=[NAME[d] for d in ALL])
@pytest.mark.parametrize("n,dims", GLUE_DIMS, ids=GLUE_IDS)
@pytest.mark.parametrize("width", WIDTHS, ids=WIDTH_IDS)
def test_copy_channels_and_add(width, n, dims, dt):
    g = torch.Generator().manual_seed(width[0] + width[1][0] + sum(dims))
    c, (a, b), want = _width_case(width, dt, n, dims, g, 2)
    dst = Slab(n, c, dims, width[2], dt)
    assert _vec(dt, c, a, dst) == want and _vec(dt, c, a, b, dst) == want, (want, width)
    assert a.ld != dst.ld
    _geom(dt, n, c, dims, want, 16)
    da, db, dd = a.desc(), b.desc(), dst.desc()
    code = N.dtype_code(dt)
    N.check(N.lib.ru3d_copy_channels(N.ref(da), N.ref(dd), code, N.stream(DEV)), "copy_channels")
    assert torch.equal(dst.t.view(INT[dt]).cpu(), a.t.view(INT[dt]).cpu()), "copy is not bit-equal to its source"
    dst.guard_ok("copy_channels")
    dst = Slab(n, c, dims, width[2], dt)
    dd = dst.desc()
    N.check(N.lib.ru3d_add(N.ref(da), N.ref(db), N.ref(dd), code, N.stream(DEV)), "add")
    ref = (a.t.cpu().float() + b.t.cpu().float()).to(dt)          # one fp32 add, one rounding
    assert torch.equal(dst.t.cpu().view(INT[dt]), ref.view(INT[dt])), "add is not round(float(a) + float(b))"
    for s in (dst, a, b):
        s.guard_ok("add")


def _cast_values(dt, shape, g):
    """random values with, in front, the ones a conversion gets wrong: ties to even in both directions, signed zeros, the
    largest finite value of the target, and (fp16) subnormal magnitudes with their own ties"""
    fi = torch.finfo(dt)
    u = fi.eps                       # spacing at 1.0
    special = [0.0, -0.0, fi.max, -fi.max, 1.0 + u / 2, 1.0 + 3 * u / 2, -(1.0 + u / 2), -(1.0 + 3 * u / 2), 1.0 + u / 2 + u / 4096,
               1.0 + u / 2 - u / 4096, 2.0 - u / 4, fi.max * (1 - u / 8)]
    if dt == FP16:
        special += [2.0 ** -14, 2.0 ** -14 * (1 - u / 4), 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, -(2.0 ** -25), 2.0 ** -25 * 1.0001, 5 * 2.0 ** -25, 2.0 ** -14 - 2.0 ** -25,
                    2.0 ** -26, 1023.5 * 2.0 ** -24, 7e-6, -3.3e-7]
    x = torch.randn(shape, generator=g) * 3.0
    flat = x.permute(0, 2, 3, 4, 1).reshape(-1)
    k = min(len(special), flat.numel())
    flat[:k] = torch.tensor(special[:k], dtype=torch.float32)
    return flat.view(shape[0], shape[2], shape[3], shape[4], shape[1]).permute(0, 4, 1, 2, 3)


CAST_CASES = [(2, 32, (9, 10, 11), (44, 4), (33, 1)), (1, 15, (1, 1, 3), (17, 1), (19, 3)), (2, 3, (4, 5, 6), None, (5, 1)),
              (1, 32, (41, 40, 40), None, None)]          # the last: 2 099 200 elements > 8192 x 256, a second lap


@pytest.mark.parametrize("dt", [BF16, FP16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("n,c,dims,lsrc,ldst", CAST_CASES, ids=["c32", "c15_v3", "c3_ld3to5", "second_lap"])
def test_cast_f32(n, c, dims, lsrc, ldst, dt):
    g = torch.Generator().manual_seed(n + c + sum(dims))
    xv = _cast_values(dt, (n, c) + dims, g)
    src = Slab(n, c, dims, lsrc, FP32, xv)
    dst = Slab(n, c, dims, ldst, dt)
    ds, dd = src.desc(), dst.desc()
    N.check(N.lib.ru3d_cast_f32(N.ref(ds), N.ref(dd), N.dtype_code(dt), N.stream(DEV)), "cast_f32")
    ref = xv.to(dt)
    got = dst.t.cpu()
    bad = (got.view(torch.int16) != ref.view(torch.int16))
    assert not bool(bad.any()), "cast_f32 != .to(%s) at %d elements, first: %r -> %r, want %r" % (
        NAME[dt], int(bad.sum()), float(xv[bad][0]), float(got[bad][0]), float(ref[bad][0]))
    dst.guard_ok("cast_f32 dst")
    src.guard_ok("cast_f32 src")


@pytest.mark.parametrize("dt", ALL, ids=[NAME[d] for d in ALL])
@pytest.mark.parametrize("n,dims", GLUE_DIMS, ids=GLUE_IDS)
@pytest.mark.parametrize("width", WIDTHS, ids=WIDTH_IDS)
def test_pointwise(width, n, dims, dt):
    """ru3d_pointwise ops 0-3 against the float64 formulas of the comment above pointwise_kernel; b in [-8, 8]."""
    g = torch.Generator().manual_seed(width[0] + width[1][1] + sum(dims))
    c, (a, cc), want = _width_case(width, dt, n, dims, g, 2)
    b = Slab(n, c, dims, width[1], dt, torch.rand((n, c) + dims, generator=g) * 16.0 - 8.0)
    act = Slab(n, c, dims, width[1], dt, torch.nn.functional.leaky_relu(a.t.cpu().float(), S32))   # op 3: the lrelu OUTPUT
    _geom(dt, n, c, dims, want, 16)
    A, B, C, L = a.f64(), b.f64(), cc.f64(), act.f64()
    sg = torch.sigmoid(B)
    o3 = torch.where(L > 0, C, (C * S32).float().double())          # a select and one fp32 multiply
    refs = {0: (torch.nn.functional.leaky_relu(A, S32),), 1: (A * sg,), 2: (C * sg, C * A * sg * (1 - sg)), 3: (o3, o3 + B)}
    code = N.dtype_code(dt)
    for op in (0, 1, 2, 3):
        o1 = Slab(n, c, dims, width[2], dt)
        o2 = Slab(n, c, dims, width[1], dt) if op >= 2 else None
        first = act if op == 3 else a
        operands = [first, b if op >= 1 else None, cc if op >= 2 else None, o1, o2]
        assert _vec(dt, c, *operands) == want, (op, want, width)
        ds = [s.desc() if s is not None else None for s in operands]
        N.check(N.lib.ru3d_pointwise(op, N.ref(ds[0]), N.ref(ds[1]), N.ref(ds[2]), N.ref(ds[3]), N.ref(ds[4]), SLOPE, code,
                                     N.stream(DEV)), "pointwise")
        _close_out(dt, o1.t, refs[op][0], "pointwise op %d o1" % op)
        if op >= 2:
            _close_out(dt, o2.t, refs[op][1], "pointwise op %d o2" % op)
        if op == 3:
            assert torch.equal(o1.f64(), o3.to(dt).double()), "op 3 o1 is a select and one multiply: bit-equal"
        for s in operands:
            if s is not None:
                s.guard_ok("pointwise op %d" % op)


@pytest.mark.parametrize("dt", ALL, ids=[NAME[d] for d in ALL])
@pytest.mark.parametrize("v", [31, 32, 33, 1000])
@pytest.mark.parametrize("c", [5, 33, 64])
def test_repack_pitched(c, v, dt):
    """ncdhw_to_ndhwc into, and ndhwc_to_ncdhw out of, a pitched channel slice: partial 32 x 32 tiles on both axes."""
    n, dims = 2, ((10, 10, 10) if v == 1000 else (1, 1, v))
    g = torch.Generator().manual_seed(c + v)
    xv = torch.randn((n, c) + dims, generator=g) * 2.0
    x = xv.to(DEV).contiguous()
    dst = Slab(n, c, dims, (c + 3, 2), dt)
    dd = dst.desc()
    code = N.dtype_code(dt)
    N.check(N.lib.ru3d_ncdhw_to_ndhwc(N.ptr(x), N.ref(dd), code, N.stream(DEV)), "ncdhw_to_ndhwc")
    assert torch.equal(dst.t.cpu().view(INT[dt]), xv.to(dt).view(INT[dt])), "ncdhw_to_ndhwc != x.to(dt)"
    dst.guard_ok("ncdhw_to_ndhwc")
    back = torch.full((n, c) + dims, float("nan"), dtype=torch.float32, device=DEV)
    N.check(N.lib.ru3d_ndhwc_to_ncdhw(N.ref(dd), N.ptr(back), code, N.stream(DEV)), "ndhwc_to_ncdhw")
    assert back.is_contiguous() and torch.equal(back.cpu(), xv.to(dt).float()), "ndhwc_to_ncdhw != stored values"


# --------------------------------------------------------------------------- 6. launch sequences
# What every entry point of the family launches, in order, as the launch log reports it.  n = 2, C = 12, (3, 5, 7) at dense
# pitch: width 4 in every type, and C % 8 != 0 keeps the backward on norm.hip's launches.
LOG_SHAPE = (2, 12, (3, 5, 7))
_IN_BWD = "in_lrelu_bwd_reduce;in_lrelu_bwd_finalize;in_lrelu_bwd_apply"


def _call_stats(o):
    return N.lib.ru3d_instnorm_stats(o["y"], None, o["mean"], o["scale"], o["ws"], o["nbytes"], IN_EPS, o["code"], o["st"])


def _call_in_fwd(o):
    return N.lib.ru3d_in_lrelu_fwd(o["y"], o["mean"], o["scale"], o["res"], o["out"], SLOPE, o["code"], o["st"])


def _call_in_bwd(o, gpre, dsum):
    return N.lib.ru3d_in_lrelu_bwd(o["gout"], o["act"], o["y"], o["mean"], o["scale"], o["dy"], o["gpre"] if gpre else None,
                                   o["ws"], o["nbytes"], SLOPE, 0, None, o["dsum"] if dsum else None, o["code"], o["st"])


def _call_in_bwd_apply(o):
    return N.lib.ru3d_in_lrelu_bwd_apply(o["gout"], o["act"], o["mean"], o["scale"], o["m12"], o["dy"], SLOPE, 0, o["code"],
                                         o["st"])


def _call_bn_stats_pool(o):
    return N.lib.ru3d_batchnorm_stats_pool(o["y"], None, o["pooled"], o["ws"], o["nbytes"], o["code"], o["st"])


def _call_affine_fwd(o):
    return N.lib.ru3d_affine_lrelu_fwd(o["y"], o["scale"], o["mean"], o["res"], o["out"], SLOPE, o["code"], o["st"])


def _call_bn_bwd_pool(o):
    return N.lib.ru3d_batchnorm_bwd_pool(o["gout"], o["act"], o["y"], o["scale"], o["mean"], o["gpre"], o["pooled"], o["ws"],
                                         o["nbytes"], SLOPE, o["code"], o["st"])


def _call_bn_bwd_apply(o):
    return N.lib.ru3d_batchnorm_bwd_apply(o["gout"], o["y"], o["scale"], o["mean"], o["scale"], o["pooled"], 210.0, o["dy"],
                                          o["ws"], o["nbytes"], 0, o["code"], o["st"])


def _call_pointwise(o, op):
    return N.lib.ru3d_pointwise(op, o["act"], o["y"] if op else None, o["gout"] if op else None, o["out"],
                                o["dy"] if op else None, SLOPE, o["code"], o["st"])


LAUNCHES = [
    ("instnorm_stats", _call_stats, "instnorm_stats;instnorm_stats_finalize"),
    ("in_lrelu_fwd", _call_in_fwd, "in_lrelu_fwd"),
    ("in_lrelu_bwd", lambda o: _call_in_bwd(o, False, False), _IN_BWD),
    ("in_lrelu_bwd_gpre", lambda o: _call_in_bwd(o, True, False), _IN_BWD),
    ("in_lrelu_bwd_dysum", lambda o: _call_in_bwd(o, False, True), _IN_BWD + ";in_lrelu_bwd_dysum_finalize"),
    ("in_lrelu_bwd_gpre_dysum", lambda o: _call_in_bwd(o, True, True), _IN_BWD + ";in_lrelu_bwd_dysum_finalize"),
    ("in_lrelu_bwd_apply", _call_in_bwd_apply, "in_lrelu_bwd_apply"),
    ("batchnorm_stats_pool", _call_bn_stats_pool, "batchnorm_stats_reduce;batchnorm_stats_pool"),
    ("affine_lrelu_fwd", _call_affine_fwd, "affine_lrelu_fwd"),
    ("batchnorm_bwd_pool", _call_bn_bwd_pool, "batchnorm_bwd_reduce;batchnorm_bwd_pool"),
    ("batchnorm_bwd_apply", _call_bn_bwd_apply, "batchnorm_bwd_means;batchnorm_bwd_apply"),
    ("channel_sum", lambda o: N.lib.ru3d_channel_sum(o["y"], o["dsum"], o["ws"], o["nbytes"], o["code"], o["st"]),
     "channel_sum;channel_sum_finalize"),
    ("copy_channels", lambda o: N.lib.ru3d_copy_channels(o["y"], o["out"], o["code"], o["st"]), "copy_add"),
    ("add", lambda o: N.lib.ru3d_add(o["y"], o["res"], o["out"], o["code"], o["st"]), "copy_add"),
    ("pointwise_op0", lambda o: _call_pointwise(o, 0), "pointwise"),
    ("pointwise_op3", lambda o: _call_pointwise(o, 3), "pointwise"),
]


def _log_operands(dt):
    """descriptors and pointers of one set of dense operands, built once per dtype; the inputs are never modified"""
    key = ("launch log", dt)
    if key not in _INPUTS:
        n, c, dims = LOG_SHAPE
        g = torch.Generator().manual_seed(12)
        rnd = lambda: torch.randn((n, c) + dims, generator=g)   # noqa: E731
        slabs = {"y": Slab(n, c, dims, None, dt, rnd() * 1.5 + 0.2), "res": Slab(n, c, dims, None, dt, rnd() * 0.5),
                 "gout": Slab(n, c, dims, None, dt, rnd()), "act": Slab(n, c, dims, None, dt, rnd()),
                 "out": Slab(n, c, dims, None, dt), "dy": Slab(n, c, dims, None, dt), "gpre": Slab(n, c, dims, None, dt)}
        assert _vec(dt, c, *slabs.values()) == 4
        assert _not_small(dt, c, dims, *slabs.values())
        descs = {k: s.desc() for k, s in slabs.items()}
        nbytes = N.lib.ru3d_reduce_workspace_bytes(N.ref(descs["y"]))
        tens = {"mean": torch.randn(n * c, generator=g).to(DEV), "scale": (torch.rand(n * c, generator=g) + 0.5).to(DEV),
                "m12": torch.randn(n * c * 2, generator=g).to(DEV), "dsum": torch.empty(c, dtype=torch.float32, device=DEV),
                "pooled": torch.randn(2 * c, generator=g).double().to(DEV), "ws": _ws(nbytes)}
        o = {k: N.ref(d) for k, d in descs.items()}
        o.update({k: N.ptr(t) for k, t in tens.items()})
        o.update(code=N.dtype_code(dt), st=N.stream(DEV), nbytes=nbytes)
        _INPUTS[key] = (o, slabs, descs, tens)          # the descriptors and tensors stay alive with their pointers
    return _INPUTS[key][0]


@pytest.mark.parametrize("dt", [BF16, FP32], ids=["bf16", "f32"])
@pytest.mark.parametrize("name,call,want", LAUNCHES, ids=[case[0] for case in LAUNCHES])
def test_launch_sequence(name, call, want, dt):
    o = _log_operands(dt)
    N.lib.ru3d_launch_log_begin()
    rc = call(o)
    got = N.lib.ru3d_launch_log_end().decode()
    N.check(rc, name)
    torch.cuda.synchronize()
    assert got == want


def test_launch_sequence_head_in_bwd():
    """ru3d_head_in_bwd on the smallest shape it takes and in_small_mode refuses (C = 32, 3 classes, V = 8400 > 8192):
    head_bwd_launch's two names, then the head's own three."""
    n, c, hc, dims = 1, 32, 3, (21, 20, 20)
    g = torch.Generator().manual_seed(32)
    z = ops.as_input((torch.randn((n, c) + dims, generator=g)).to(DEV), BF16)
    y = ops.as_input((torch.randn((n, c) + dims, generator=g) * 1.5 + 0.2).to(DEV), BF16)
    gy = N.to_ndhwc((torch.randn((n, hc) + dims, generator=g) * 1e-2).to(DEV))
    hw = (torch.randn(hc, c, 1, 1, 1, generator=g) * 0.3).to(DEV)
    mean, scale = ops.in_stats(y)
    N.lib.ru3d_launch_log_begin()
    out = ops.head_in_bwd(z, gy, hw, True, y, mean, scale)
    got = N.lib.ru3d_launch_log_end().decode()
    torch.cuda.synchronize()
    assert out is not None, "no fused kernel"
    assert got == "head_bwd_wgrad;head_bwd_finalize;head_in_bwd_reduce;head_in_bwd_finalize;head_in_bwd_apply"
