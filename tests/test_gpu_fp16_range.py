"""fp16's own edges in the conv family: the second compilation of every kernel (-DRU3D_STORAGE_F16) at the two ends of
the format's range.  The routing tables themselves run in both storage types in tests/test_gpu_s1_routing.py and
tests/test_gpu_wgrad_routing.py; every case here first asserts the launch log against the same tables.

  store overflow   one case per store epilogue.  Operands fp16-rounded and scaled so that the float64 reference has a
                   standard deviation near 3e4 (x about 4, w about 3e4 / (4 sqrt(K)): both far inside the range), no bias.
                   Expected: the reference rounded once to fp16 by torch.  With t = 65520, the first value that rounds to
                   inf: |ref| > t (1 + 2^-8) must be +-inf with the reference's sign, |ref| < t (1 - 2^-8) must be finite
                   and within the routing tolerance, the band in between is excluded.  The band is 8 x the fp16 half-ulp
                   at t, far above the fp32 accumulation noise of these sums (about sqrt(K) 2^-24 relative, K <= 27 * 512).
                   The finite side is held against the exact value, element by element: half an ulp of the element
                   (the one rounding) + 8 sqrt(K) 2^-23 std(ref) + 1e-3 (eight deviations of the accumulation noise: K
                   additions, each off by up to an fp32 ulp of a partial sum - the MFMA's adder is not promised to round
                   to nearest - and the partial sums are of the tensor's size whatever the element's; 0.2 to 3.3), and
                   the routing tests' 2^-11 of the largest element + 1e-3 over the whole tensor.
                   The residual forms add a residual of standard deviation 16, largest value under 128, half the
                   band's half-width (asserted): which side of the band an element is on is then decided by the conv
                   value alone, whether a kernel rounds the conv value before it adds the residual (the sliding
                   kernels do) or not.  Their finite side allows both roundings: half an ulp of the conv value + half
                   an ulp of the sum, against the exact conv + res, and 1.5 x 2^-11 of the largest element overall.
                   Against round(round(conv) + res) instead, a correct kernel whose fp32 sum sits across a rounding
                   boundary from the float64 one is a whole ulp off after the first rounding and can be two after the
                   second: 64 at 65 000, where 1.5 x 2^-11 of the largest finite element is 47.8 (seen: 64 on
                   pc_w16_ragged, 48 on slide32_res and pc4_res) - so the two roundings are in the bound, not in
                   the expected value.
                   Checked on the host from the reference alone, before any launch: at most 1 % of the elements in the
                   band, at least 1 % overflow, at least half finite.  No NaN anywhere.

  subnormal exact  dy = k 2^-24 with integer k uniform in [-kmax, kmax]: exact fp16 subnormals; weights (input gradient)
                   or x (weight gradient) uniform in {-2 .. 2}.  Every product is an integer multiple of 2^-24 of at most
                   2 kmax units and every partial sum, in any order, stays below 2 kmax T < 2^24 units (T = terms per
                   output; asserted from the shapes), so fp32 accumulation is exact: the weight gradient is torch.equal
                   to the float64 sum and the input gradient to the float64 sum rounded once to fp16, subnormal results
                   included.  kmax = 255 where the bound allows it; the two sliding weight-gradient cases sum T = 131072
                   and 98304 positions, for which 2 * 255 * T is past 2^24, so they take the largest kmax the bound
                   allows (63 and 85) - still subnormals only, still every position.  A flush of subnormal inputs in the
                   LDS-DMA or staging path, or of subnormal results in the store, cannot pass.

Run with `-m gpu`."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no HIP device", allow_module_level=True)

import _native as N  # noqa: E402
import _ops as ops  # noqa: E402
import test_gpu_inner_boundaries as IB  # noqa: E402
import test_gpu_s1_routing as S1  # noqa: E402
import test_gpu_wgrad_routing as WG  # noqa: E402

DEV = torch.device("cuda:0")
F = torch.nn.functional
F16 = torch.float16
EPS = S1.EPS[F16]
T_INF = 65520.0             # the first value that rounds to inf in fp16
BAND = 2.0 ** -8
TARGET_STD = 3.0e4
X_SCALE = 4.0
RES_STD, RES_MAX = 16.0, 128.0

# id -> (table, key): the stride-1 table's case as it stands there (forward or residual form), or the forward call of an
# inner-boundaries case with the name that table expects
OVERFLOW = {c: ("s1", c) for c in ("slide32", "slide32_res", "slide64", "slide64_edge_cout32", "pc4_res", "pc_w16_ragged",
                                   "sk16", "sk8_split", "conv_ws", "tile_mt1", "tile_w8_splitk")}
OVERFLOW.update({"conv_gather_mfma": ("conv", "E2"), "convt_tile_mfma": ("convt", "H"), "conv_direct_mfma": ("convt", "D"),
                 "conv_direct_ksplit": ("convt", "G")})


def _h(t):
    return t.to(F16)


@functools.lru_cache(maxsize=2)
def _overflow_case(case):
    """(x, w, res or None as fp16 host tensors, float64 conv value, names, geometry) - the population conditions are
    checked here, on the host, before anything is launched"""
    table, key = OVERFLOW[case]
    g = torch.Generator().manual_seed(len(case) + sum(map(ord, case)))
    res = None
    if table == "s1":
        n, cin, cout, dims, what, names = S1.CASES[key]
        assert what in ("fwd", "res")
        x = _h(torch.randn((n, cin) + dims, generator=g) * X_SCALE)
        w = _h(torch.randn(cout, cin, 3, 3, 3, generator=g) * (TARGET_STD / (X_SCALE * (27 * cin) ** 0.5)))
        conv = F.conv3d(x.double(), w.double(), None, padding=1)
        if what == "res":
            res = _h(torch.randn(conv.shape, generator=g) * RES_STD)
        geom = (cout, 3, 1)
    elif table == "conv":
        c = IB.CONV[key]
        assert not c["pitched"]
        xs, _ = IB._conv_shapes(c)
        k, stride, names = c["k"], c["stride"], [c["fwd"]]
        x = _h(torch.randn(xs, generator=g) * X_SCALE)
        w = _h(torch.randn(c["cout"], c["cin"], k, k, k, generator=g) * (TARGET_STD / (X_SCALE * (k ** 3 * c["cin"]) ** 0.5)))
        conv = F.conv3d(x.double(), w.double(), None, stride=stride, padding=k // 2)
        geom = (c["cout"], k, stride)
    else:
        c = IB.CONVT[key]
        assert not c["pitched"]
        xs, _ = IB._convt_shapes(c)
        names = [c["fwd"]]
        x = _h(torch.randn(xs, generator=g) * X_SCALE)
        w = _h(torch.randn(c["cin"], c["cout"], 3, 3, 3, generator=g) * (TARGET_STD / (X_SCALE * (27 * c["cin"] / 8) ** 0.5)))
        conv = F.pad(F.conv_transpose3d(x.double(), w.double(), None, stride=2, padding=1), (0, 1, 0, 1, 0, 1))
        geom = (c["cout"], 3, 2)
    assert float(x.abs().max()) < 64 and float(w.abs().max()) < 32768, "operands not well inside the fp16 range"
    if res is not None:
        assert float(res.abs().max()) < RES_MAX
    a = conv.abs()
    over, under = a > T_INF * (1 + BAND), a < T_INF * (1 - BAND)
    band = 1.0 - (over | under).double().mean().item()
    print("OVERFLOW %s: std %.4g, band %.4f %%, overflow %.3f %%, finite %.3f %%" % (
        case, conv.std().item(), 100 * band, 100 * over.double().mean().item(), 100 * under.double().mean().item()))
    assert band <= 0.01 and over.double().mean().item() >= 0.01 and under.double().mean().item() >= 0.5
    return x, w, res, conv, names, table, geom


@pytest.mark.parametrize("case", sorted(OVERFLOW))
def test_store_overflow_goes_to_inf(case):
    x, w, res, conv, names, table, (cout, k, stride) = _overflow_case(case)
    xd = ops.as_input(x.float().to(DEV), F16)
    rd = ops.as_input(res.float().to(DEV), F16) if res is not None else None
    role = N.ROLE_CONVT_FWD if table == "convt" else N.ROLE_CONV_FWD
    pw = ops.pack_weight(w.float().to(DEV), role, F16, stride) if table != "convt" else ops.pack_weight(w.float().to(DEV), role, F16)
    with ops.launch_log() as log:
        if table == "convt":
            got = ops.convt_fwd(xd, pw, None, cout)
        else:
            got = ops.conv_fwd(xd, pw, None, cout, k, stride, res=rd)
    print("ROUTE %s %s" % (case, log.names))
    assert log.names == names
    got = got.float().cpu()
    assert got.shape == conv.shape
    assert not bool(torch.isnan(got).any()), "%d NaN" % int(torch.isnan(got).sum())
    a = conv.abs()
    over, under = a > T_INF * (1 + BAND), a < T_INF * (1 - BAND)
    inf_ok = torch.isinf(got[over]) & (torch.sign(got[over]) == torch.sign(conv[over]).float())
    assert bool(inf_ok.all()), "%d of %d overflowing elements are not inf of the reference's sign (saturated?)" % (
        int((~inf_ok).sum()), int(over.sum()))
    assert bool(torch.isfinite(got[under]).all()), "%d elements under the band are not finite" % int(
        (~torch.isfinite(got[under])).sum())
    # the finite side, against the exact value: one rounding of the conv value (and one more of the sum with the residual)
    # plus the accumulation noise, element by element - and the routing tests' figure for the whole tensor on top
    exact = conv if res is None else conv + res.double()
    terms = k ** 3 * x.shape[1]
    # the noise of K fp32 additions is that of the partial sums, whose size is the tensor's deviation, not the element's
    noise = 8 * terms ** 0.5 * 2.0 ** -23 * conv.std().item()
    bound = _half_ulp(conv) + (0 if res is None else _half_ulp(exact)) + noise + 1e-3
    err = (got.double() - exact).abs()
    worst = (err / bound)[under].max().item()
    lim = 1e-3 + (EPS if res is None else 1.5 * EPS) * exact[under].abs().max().item()
    print("OVERFLOW %s: largest finite-side error %.4g (routing limit %.4g), at most %.3f of the element's own bound; "
          "%d inf, %d in the band" % (case, err[under].max().item(), lim, worst, int(over.sum()), int((~over & ~under).sum())))
    assert worst <= 1.0, "%s: finite side: %d elements past their rounding bound, worst %.3f x" % (
        case, int((err > bound)[under].sum()), worst)
    assert err[under].max().item() <= lim, "%s: finite side: max err %.4g > %.4g" % (case, err[under].max().item(), lim)


def _half_ulp(v):
    """half the spacing of fp16 at |v| (normal numbers)"""
    return torch.pow(2.0, torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -14))) - 11)


# ---------------------------------------------------------------------------------------------------------- subnormals
UNITS = 2.0 ** -24
SUB_DGRAD = ["slide64_dgrad", "pc4_dgrad"]
SUB_WGRAD = ["slide", "slide_light", "s2_dma2", "tile_w8"]


def _kmax(terms):
    """largest |k| <= 255 for which 2 |k| `terms` - the bound on any partial sum, in units of 2^-24 - stays below 2^24"""
    kmax = min(255, (2 ** 24 - 1) // (2 * terms))
    assert kmax >= 1 and 2 * kmax * terms < 2 ** 24
    return kmax


def _subnormals(shape, kmax, g):
    t = torch.randint(-kmax, kmax + 1, shape, generator=g).double() * UNITS
    assert bool((t.to(F16).double() == t).all()) and float(t.abs().max()) < 2.0 ** -14     # exact, and subnormal
    return t


@pytest.mark.parametrize("case", SUB_DGRAD)
def test_subnormal_gradients_input_gradient_exact(case):
    n, cin, cout, dims, what, names = S1.CASES[case]
    assert what == "dgrad"
    d, h, w = dims
    g = torch.Generator().manual_seed(len(case) + cin + cout)
    kmax = _kmax(27 * cout)
    assert kmax == 255
    gy = _subnormals((n, cout) + dims, kmax, g)
    wt = torch.randint(-2, 3, (cout, cin, 3, 3, 3), generator=g).double()
    ref = F.conv_transpose3d(gy, wt, None, padding=1)
    assert bool((ref / UNITS == (ref / UNITS).round()).all()) and float(ref.abs().max()) < 2.0 ** 24 * UNITS
    want = ref.float().to(F16)          # exact in fp32, then the one rounding
    assert bool((want.double() != ref).any()) and bool(((want != 0) & (want.abs() < 2.0 ** -14)).any()), \
        "the case holds neither a rounded nor a subnormal result"
    pw = ops.pack_weight(wt.float().to(DEV), N.ROLE_CONV_DGRAD, F16, 1)
    gyd = ops.as_input(gy.float().to(DEV), F16)
    assert torch.equal(gyd.cpu().double(), gy), "the subnormals did not reach the device intact"
    with ops.launch_log() as log:
        got = ops.conv_dgrad(gyd, pw, (n, cin, d, h, w), 3, 1)
    print("ROUTE %s %s" % (case, log.names))
    assert log.names == names
    got = got.cpu()
    bad = int((got != want).sum())
    print("SUBNORMAL %s: %d of %d entries differ; %d subnormal results" % (
        case, bad, want.numel(), int(((want != 0) & (want.abs() < 2.0 ** -14)).sum())))
    assert torch.equal(got, want), "%d of %d entries differ" % (bad, want.numel())


@pytest.mark.parametrize("case", SUB_WGRAD)
def test_subnormal_gradients_weight_gradient_exact(case):
    what, _, n, cin, cout, dims, k, stride, names = WG.CASES[case]
    assert what == "conv"
    ydims = tuple((s - 1) // stride + 1 for s in dims)
    terms = n * ydims[0] * ydims[1] * ydims[2]
    kmax = _kmax(terms)
    g = torch.Generator().manual_seed(len(case) + cin + cout + sum(dims))
    xv = torch.randint(-2, 3, (n, cin) + dims, generator=g).double()
    gy = _subnormals((n, cout) + ydims, kmax, g)
    ref = WG._wgrad_ref(xv, gy, k, stride)
    assert bool((ref / UNITS == (ref / UNITS).round()).all()) and float(ref.abs().max()) < 2.0 ** 24 * UNITS
    want = ref.float()
    assert bool((want.double() == ref).all())
    x = ops.as_input(xv.float().to(DEV), F16)
    dy = ops.as_input(gy.float().to(DEV), F16)
    assert torch.equal(dy.cpu().double(), gy), "the subnormals did not reach the device intact"
    with ops.launch_log() as log:
        got = ops.conv_wgrad(x, dy, k, stride)
    print("ROUTE %s %s" % (case, log.names))
    assert log.names == names
    got = got.cpu()
    bad = int((got != want).sum())
    print("SUBNORMAL %s: kmax %d, %d terms, %d of %d entries differ" % (case, kmax, terms, bad, want.numel()))
    assert torch.equal(got, want), "%d of %d entries differ" % (bad, want.numel())
