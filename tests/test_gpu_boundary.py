"""The boundary-loss kernels of csrc/boundary.hip on a real MI355X: the signed distance maps (integer squares and float
maps, every element), the loss modules BoundaryLoss and HybirdBoundaryLoss (value and gradient down to the logits),
sample isolation, determinism, the deferred label check, the captured training step with a boundary weight that is
rescheduled between replays, and the bit equality with HybirdLoss at weight 0.

Reference of the maps: the numpy twin in loss.py (signed_distance_map on host tensors, scipy's exact transform), held
to an all-pairs brute force by tests/test_host_boundary.py.  Reference of the losses: the torch twin (BoundaryLoss on
host tensors) evaluated in float64 on the float32 inputs, the gradient by float64 autograd; the Hybird part as in
tests/test_gpu_loss_kernels.py.

The kernels' constants (boundary.hip): the two scan kernels run 512 threads (BD_THREADS) over an LDS tile of one whole
column of the scanned axis (B, then A) times T columns of z; T is the largest power of two with T / 2 < Z, at most 32
(BD_MAX_COLS), halved until L * T <= 8192 (BD_TILE) for a scanned axis of L voxels.  A workgroup walks its tile 512
elements a trip, so a trip covers 512 / T voxels of the scanned axis.  The Z pass reads 64-voxel packed words.  The
shapes below are derived from these:
  BASE (12, 10, 9)        T = 16, one tile of z, one trip
  TILE_PLUS_ONE (17, 17, 33)   T = 32: a second tile of z with a single column, and 17 * 32 = 544 elements: one voxel of
                          each scanned axis falls into a second trip
  LINE70 / LINE130 (1, 1, 70 / 130)   rows of two and three packed words
  SINGLE (1, 1, 1)        always degenerate
  BEYOND (129, 65, 5)     T = 8, 64 voxels a trip: one beyond two trips along A, one beyond one trip along B
  LONG (300, 2, 40)       300 * 32 > 8192: the A pass drops to T = 16 (three tiles of z) while the B pass keeps T = 32
  CORNER (40, 9, 70)      the only voxel of class 1 in one corner, the only voxel of class 2 in the opposite one: every
                          scan that can run to its hard bound does

Tolerances:
  * maps: equality, every element.
  * value: |err| <= 2e-6 * max(1, |ref|), the bound of the fused losses.
  * gradient, element by element: |err| <= 2e-5 * |ref| + F * max|ref|, F twice what the SAME chain evaluated in
    float32 on the host (the twin on .float() inputs, the Hybird part in float32 too) misses the float64 reference by,
    measured for each case on the host as the worst element error over max|ref| and rounded up to two digits:
        c2 boundary ncdhw 2.80e-7, c2 hybird a=0.5 ndhwc u8 1.69e-7, c3 boundary ndhwc 2.82e-7,
        c3 hybird a=0.01 ncdhw 2.29e-7, c3 hybird a=0.5 ncdhw 2.37e-7, c3 hybird a=1.0 ncdhw 3.51e-7,
        c3 boundary classes=(2,) 2.44e-7, c3 hybird weighted 2.43e-7, c3 hybird tile+1 3.11e-7, c2 boundary line 2.34e-7,
        c3 hybird upstream 1024 2.37e-7, the bf16 case 1.82e-7 (the float32 gradient of the widened logits, which is
        what the floor is applied to; the bf16 gradient is that one rounded once).
    The floors stand next to the cases (LOSS_CASES, F_BF16).
Run with `-m gpu`."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no HIP device", allow_module_level=True)

import graph  # noqa: E402
import loss as L  # noqa: E402
import network  # noqa: E402
import optim  # noqa: E402
import _ops as ops  # noqa: E402
from oracle import unet_oracle as O  # noqa: E402

DEV = torch.device("cuda:0")
VALUE_TOL = 2e-6
GRAD_REL = 2e-5
BASE = (12, 10, 9)
TILE_PLUS_ONE = (17, 17, 33)
LINE70 = (1, 1, 70)
LINE130 = (1, 1, 130)
SINGLE = (1, 1, 1)
BEYOND = (129, 65, 5)
LONG = (300, 2, 40)
CORNER = (40, 9, 70)


# ------------------------------------------------------------------------------------------------ inputs
def blob_labels(n, shape, c, seed):
    """Seeded labels in [0, c): a coarse random grid enlarged by nearest neighbour, so there are blobs, not salt."""
    g = torch.Generator().manual_seed(seed)
    coarse = torch.randint(0, c, (n,) + tuple((s + 2) // 3 for s in shape), generator=g)
    y = coarse.repeat_interleave(3, 1).repeat_interleave(3, 2).repeat_interleave(3, 3)
    y = y[:, :shape[0], :shape[1], :shape[2]].contiguous()
    salt = torch.rand(y.shape, generator=g) < 0.05
    return torch.where(salt, torch.randint(0, c, y.shape, generator=g), y)


@functools.lru_cache(maxsize=None)
def map_case(name):
    """name -> labels (N, A, B, Z) int64 with values in [0, 3)."""
    if name == "base":
        return blob_labels(2, BASE, 3, 11)
    if name == "tile+1":
        return blob_labels(1, TILE_PLUS_ONE, 3, 13)
    if name == "line70":
        y = blob_labels(2, LINE70, 3, 15)
        y[0, 0, 0, 60:68] = 1                            # a run across the word boundary
        return y
    if name == "line130":
        y = torch.zeros((1,) + LINE130, dtype=torch.int64)
        y[0, 0, 0, 0] = 1                                # the nearest voxel of the other kind is two words away
        y[0, 0, 0, 129] = 2
        return y
    if name == "single":
        return torch.ones((1,) + SINGLE, dtype=torch.int64)
    if name == "beyond":
        return blob_labels(1, BEYOND, 3, 17)
    if name == "long":
        return blob_labels(1, LONG, 3, 19)
    if name == "corner":
        y = torch.zeros((1,) + CORNER, dtype=torch.int64)
        y[0, 0, 0, 0] = 1
        y[0, -1, -1, -1] = 2
        return y
    raise KeyError(name)


MAP_CASES = ["base", "tile+1", "line70", "line130", "single", "beyond", "long", "corner"]


@functools.lru_cache(maxsize=None)
def twin_squares(name, classes):
    return L.signed_distance_map(map_case(name), 3, classes=classes, squared=True)


def phi_of(d2):
    """float32(sqrt(float64(d2))) with the sign rule."""
    root = d2.abs().double().sqrt().float()
    return torch.where(d2 < 0, -(root - 1.0), root)


def assert_maps(labels_dev, classes, want, what):
    sq = L.signed_distance_map(labels_dev, 3, classes=classes, squared=True)
    assert sq.is_cuda and sq.dtype == torch.int32 and sq.shape == want.shape, what
    sq = sq.cpu()
    print("%s: %d of %d squares differ, largest |d2| %d" % (what, int((sq != want).sum()), want.numel(),
                                                            int(want.abs().max())))
    assert torch.equal(sq, want), what
    phi = L.signed_distance_map(labels_dev, 3, classes=classes)
    assert phi.is_cuda and phi.dtype == torch.float32 and phi.shape == want.shape, what
    assert torch.equal(phi.cpu(), phi_of(want)), what


# ------------------------------------------------------------------------------------------------ the maps
@pytest.mark.parametrize("name", MAP_CASES)
def test_maps_equal_the_twin(name):
    y = map_case(name)
    for classes in ((2,), (1, 2), (2, 1)):
        want = twin_squares(name, classes)
        for dtype in (torch.uint8, torch.int64):
            assert_maps(y.to(dtype).to(DEV), classes, want, "%s %s %s" % (name, classes, dtype))
    assert torch.equal(twin_squares(name, (1, 2)).flip(1), twin_squares(name, (2, 1)))      # the slots follow `classes`
    if name == "single":
        assert not twin_squares(name, (1, 2)).any()
    if name == "corner":
        a, b, z = CORNER
        assert int(twin_squares(name, (1,))[0, 0, -1, -1, -1]) == (a - 1) ** 2 + (b - 1) ** 2 + (z - 1) ** 2


@pytest.mark.parametrize("name", ["beyond", "long"])
def test_maps_with_a_capped_grid(name):
    """The pack kernel's grid is capped at 8 blocks a CU of the budget, the two scan kernels' at 4 (tiles of 32 KiB of
    LDS).  "beyond" (129, 65, 5), two classes: 8385 words = 2097 pack blocks, 2 * 129 and 2 * 65 tiles at the least; "long"
    (300, 2, 40): 600 words = 150 pack blocks, 2 * 300 tiles at the least in the first scan.  With the whole chip the scans
    get up to 1024 blocks and only the pack of "beyond" meets its cap (2048); under a budget of 8 CUs the caps are 64 and
    32, so these loops stride.  The same squares and maps as the twin, as in test_maps_equal_the_twin."""
    import _native as N
    y = map_case(name)
    try:
        assert N.lib.ru3d_set_cu_budget(8) == 0
        for classes in ((1, 2), (2,)):
            assert_maps(y.to(torch.uint8).to(DEV), classes, twin_squares(name, classes), "%s %s under 8 CUs" % (name, classes))
    finally:
        N.lib.ru3d_set_cu_budget(0)
    assert N.lib.ru3d_get_cu_budget() == torch.cuda.get_device_properties(DEV).multi_processor_count


def test_default_classes_int32_labels_and_a_strided_view():
    y = map_case("base")
    want = twin_squares("base", (1, 2))
    assert torch.equal(L.signed_distance_map(y.to(DEV), 3, squared=True).cpu(), want)
    assert torch.equal(L.signed_distance_map(y.to(torch.int32).to(DEV), 3, squared=True).cpu(), want)
    wide = torch.zeros((2, 12, 10, 18), dtype=torch.int64)
    wide[..., ::2] = y
    assert torch.equal(L.signed_distance_map(wide.to(DEV)[..., ::2], 3, squared=True).cpu(), want)


def test_degenerate_volumes_and_sample_isolation():
    y = map_case("base").clone()
    y[0][y[0] == 2] = 0                                  # class 2 absent from sample 0 only
    y[1][y[1] == 0] = 1
    y[1][y[1] == 2] = 1                                  # class 1 fills sample 1 only
    want = L.signed_distance_map(y, 3, classes=(1, 2), squared=True)
    assert not want[0, 1].any() and not want[1].any() and bool(want[0, 0].all())
    for dtype in (torch.uint8, torch.int64):
        assert_maps(y.to(dtype).to(DEV), (1, 2), want, "degenerate %s" % dtype)
    # the other sample's maps are those of that sample alone, bit for bit
    full = map_case("base")
    mixed = torch.stack((y[0], full[1]))
    for squared in (True, False):
        both = L.signed_distance_map(mixed.to(DEV), 3, squared=squared)
        for n in range(2):
            alone = L.signed_distance_map(mixed[n:n + 1].to(DEV), 3, squared=squared)
            assert torch.equal(both[n:n + 1], alone), (squared, n)
        swapped = L.signed_distance_map(mixed.flip(0).to(DEV), 3, squared=squared)
        assert torch.equal(swapped.flip(0), both), squared
        assert not bool(both[0, 1].any()), squared
        if squared:
            assert bool(both[1].ne(0).all()) and bool(both[0, 0].ne(0).all())


def test_out_of_range_labels_match_no_class():
    y = map_case("base").clone()
    holes = torch.rand(y.shape, generator=torch.Generator().manual_seed(5)) < 0.04
    as_background = torch.where(holes, torch.zeros_like(y), y)
    want = L.signed_distance_map(as_background, 3, classes=(1, 2), squared=True)
    assert torch.equal(L.signed_distance_map(torch.where(holes, torch.full_like(y, 9), y), 3, squared=True), want)
    assert_maps(torch.where(holes, torch.full_like(y, 255), y).to(torch.uint8).to(DEV), (1, 2), want, "label 255")
    assert_maps(torch.where(holes, torch.full_like(y, -3), y).to(DEV), (1, 2), want, "label -3")
    assert_maps(torch.where(holes, torch.full_like(y, 3), y).to(DEV), (1, 2), want, "label 3")


# ------------------------------------------------------------------------------------------------ comparisons
def assert_value(got, ref, what):
    got = float(got)
    print("%s: value %.9g, float64 %.9g, |err| %.3g" % (what, got, ref, abs(got - ref)))
    assert abs(got - ref) <= VALUE_TOL * max(1.0, abs(ref)), "%s: value %.9g, float64 %.9g" % (what, got, ref)


def assert_grad(got, ref, what, floor):
    got = got.detach().to("cpu", torch.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), "%s: gradient not finite" % what
    err = (got - ref).abs()
    top = float(ref.abs().max())
    print("%s: worst gradient error %.3g of max|ref| %.3g" % (what, float(err.max()) / max(top, 1e-300), top))
    tol = GRAD_REL * ref.abs() + floor * top
    bad = err > tol
    assert not bool(bad.any()), "%s: %d gradient elements off, worst %.3g of its bound (max|ref| %.3g)" % (
        what, int(bad.sum()), float((err / tol.clamp_min(1e-300)).max()), top)


# ------------------------------------------------------------------------------------------------ logit-level losses
def hybird_reference(z, y, weight_v=None):
    """HybirdLoss(gamma=2, alpha=beta=0.5, smooth=1e-7) in the dtype of z (tests/test_gpu_loss_kernels.py)."""
    n, c = z.shape[:2]
    zf = z.reshape(n, c, -1)
    yf = y.reshape(n, 1, -1)
    logp = torch.log_softmax(zf, dim=1)
    p = logp.exp()
    g = torch.zeros_like(zf).scatter_(1, yf, 1.0)
    w = torch.ones(c, dtype=z.dtype) if weight_v is None else torch.tensor(
        [float(torch.tensor(float(a), dtype=torch.float32)) for a in weight_v], dtype=z.dtype)
    w = w / w.abs().sum().clamp_min(1e-12)
    s = float(torch.tensor(1e-7, dtype=torch.float32))
    tp, sp, sg = (p * g).sum((0, 2)), p.sum((0, 2)), g.sum((0, 2))
    dice = (tp + s) / (tp + 0.5 * (sg - tp) + 0.5 * (sp - tp) + s)
    lt, pt = logp.gather(1, yf), p.gather(1, yf)
    focal = torch.zeros(c, dtype=z.dtype).index_add(0, yf.reshape(-1), (-((1.0 - pt) ** 2) * lt).reshape(-1))
    return (w * (1.0 - dice + focal * c / (n * zf.shape[2]))).sum()


def loss_reference(x, y, a, classes=None, weight_v=None, upstream=1.0, dtype=torch.float64):
    """Value and gradient by autograd through the twin, in `dtype`, on the host.  `a` as the device holds it: float32."""
    z = x.detach().cpu().float().to(dtype).contiguous().requires_grad_(True)
    yl = y.detach().cpu().long()
    bd = L.BoundaryLoss(weight_v=weight_v, classes=classes)(z, yl)
    if a is None:
        v = bd
    else:
        a32 = torch.tensor(a, dtype=torch.float32)
        v = float(1.0 - a32) * hybird_reference(z, yl, weight_v) + float(a32) * bd
    (upstream * v).backward()
    return float(v.detach()), z.grad


def loss_device(x, y, a, classes=None, weight_v=None, upstream=1.0):
    x = x.detach().requires_grad_(True)
    if a is None:
        crit = L.BoundaryLoss(weight_v=weight_v, classes=classes)
    else:
        crit = L.HybirdBoundaryLoss(boundary_weight=a, classes=classes, weight_v=weight_v)
    v = crit(x, y)
    assert v.dim() == 0 and v.is_cuda and v.dtype == torch.float32
    (v * upstream).backward()
    assert x.grad.shape == x.shape and x.grad.dtype == x.dtype and x.grad.stride() == x.stride()
    return v.detach(), x.grad.detach()


def logits_for(y, c, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn((y.shape[0], c) + tuple(y.shape[1:]), generator=g) * 2).float()


def ndhwc(x):
    return x.contiguous(memory_format=torch.channels_last_3d)


def make_case(name):
    """name -> (logits in the case's layout, labels, keyword arguments)."""
    y3, y2 = map_case("base"), map_case("base").clamp(max=1)
    if name == "c2 boundary ncdhw":
        return logits_for(y2, 2, 201), y2, dict(a=None)
    if name == "c2 hybird a=0.5 ndhwc u8":
        return ndhwc(logits_for(y2, 2, 203)), y2.to(torch.uint8), dict(a=0.5)
    if name == "c3 boundary ndhwc":
        return ndhwc(logits_for(y3, 3, 205)), y3, dict(a=None)
    if name == "c3 hybird a=0.01 ncdhw":
        return logits_for(y3, 3, 207), y3, dict(a=0.01)
    if name == "c3 hybird a=0.5 ncdhw":
        return logits_for(y3, 3, 207), y3, dict(a=0.5)
    if name == "c3 hybird a=1.0 ncdhw":
        return logits_for(y3, 3, 207), y3, dict(a=1.0)
    if name == "c3 boundary classes=(2,)":
        return logits_for(y3, 3, 209), y3, dict(a=None, classes=(2,))
    if name == "c3 hybird weighted":
        return logits_for(y3, 3, 211), y3, dict(a=0.5, weight_v=[0.2, 1.0, 3.0], classes=(2, 1))
    if name == "c3 hybird tile+1":
        yt = map_case("tile+1")
        return ndhwc(logits_for(yt, 3, 213)), yt, dict(a=0.5)
    if name == "c2 boundary line":
        yl = map_case("line70").clamp(max=1)
        return logits_for(yl, 2, 215), yl, dict(a=None)
    if name == "c3 hybird upstream 1024":
        return logits_for(y3, 3, 207), y3, dict(a=0.5, upstream=1024.0)
    raise KeyError(name)


# case -> F
LOSS_CASES = {"c2 boundary ncdhw": 5.6e-7, "c2 hybird a=0.5 ndhwc u8": 3.4e-7, "c3 boundary ndhwc": 5.7e-7,
              "c3 hybird a=0.01 ncdhw": 4.6e-7, "c3 hybird a=0.5 ncdhw": 4.8e-7, "c3 hybird a=1.0 ncdhw": 7.1e-7,
              "c3 boundary classes=(2,)": 4.9e-7, "c3 hybird weighted": 4.9e-7, "c3 hybird tile+1": 6.3e-7,
              "c2 boundary line": 4.7e-7, "c3 hybird upstream 1024": 4.8e-7}
F_BF16 = 3.7e-7


def bf16_case():
    y2 = map_case("base").clamp(max=1)
    return logits_for(y2, 2, 221).to(torch.bfloat16), y2, dict(a=0.5)


@pytest.mark.parametrize("name", sorted(LOSS_CASES))
def test_losses_value_and_gradient(name):
    x, y, kw = make_case(name)
    ref_v, ref_g = loss_reference(x, y, **kw)
    v, g = loss_device(x.to(DEV), y.to(DEV), **kw)
    assert_value(v, ref_v, name)
    assert_grad(g, ref_g, name, LOSS_CASES[name])


def test_bf16_logits():
    """The kernels read float32: 16-bit logits are widened first, and the bf16 gradient is the float32 gradient of the
    widened logits rounded once (asserted bit for bit).  That float32 gradient is held to the float64 reference at the
    gate of every other case (F_BF16); the bf16 gradient is held to the same gate carried through the rounding."""
    x, y, kw = bf16_case()
    assert x.dtype == torch.bfloat16
    ref_v, ref_g = loss_reference(x, y, **kw)
    v, g = loss_device(x.to(DEV), y.to(DEV), **kw)
    assert g.dtype == torch.bfloat16
    assert_value(v, ref_v, "bf16")
    v32, g32 = loss_device(x.float().to(DEV), y.to(DEV), **kw)
    assert torch.equal(v, v32) and torch.equal(g, g32.to(torch.bfloat16))
    assert_grad(g32, ref_g, "bf16 widened", F_BF16)
    tol = GRAD_REL * ref_g.abs() + F_BF16 * float(ref_g.abs().max())
    lo, hi = (ref_g - tol).to(torch.bfloat16).double(), (ref_g + tol).to(torch.bfloat16).double()
    got = g.cpu().double()
    assert bool(((got >= lo) & (got <= hi)).all())


def test_an_absent_class_gives_no_loss_and_no_gradient():
    y = map_case("base").clamp(max=1)                    # class 2 absent from both samples
    x = logits_for(y, 3, 225)
    v, g = loss_device(x.to(DEV), y.to(DEV), None, classes=(2,))
    assert float(v) == 0.0 and float(g.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ bit equalities
def test_boundary_weight_zero_is_hybird_loss():
    y = map_case("base")
    x = logits_for(y, 3, 231)
    for layout in ("ncdhw", "ndhwc"):
        xx = (x if layout == "ncdhw" else ndhwc(x)).to(DEV)
        crit = L.HybirdBoundaryLoss(weight_v=[1.0, 2.0, 3.0])
        crit.set_boundary_weight(0.0)
        assert crit.boundary_weight == 0.0
        a = xx.detach().requires_grad_(True)
        va = crit(a, y.to(DEV))
        va.backward()
        b = xx.detach().requires_grad_(True)
        vb = L.HybirdLoss(weight_v=[1.0, 2.0, 3.0])(b, y.to(DEV))
        vb.backward()
        assert torch.equal(va, vb), layout
        assert torch.equal(a.grad.view(torch.int32), b.grad.view(torch.int32)), layout       # the bits, signed zeros too


def test_same_input_same_bits():
    big_y = blob_labels(2, (19, 21, 70), 3, 6)
    big = logits_for(big_y, 3, 5)
    for xx, yy in ((logits_for(map_case("base"), 3, 241), map_case("base")), (big, big_y)):
        for a in (None, 0.5):
            v1, g1 = loss_device(xx.to(DEV), yy.to(DEV), a)
            v2, g2 = loss_device(xx.to(DEV), yy.to(DEV), a)
            assert torch.equal(v1, v2) and torch.equal(g1, g2)


@pytest.mark.parametrize("a", [None, 0.5])
def test_label_out_of_range_raises(a):
    y = map_case("base").clone()
    y[1, 3, 4, 5] = 3
    x = logits_for(y, 3, 251)
    L.raise_on_bad_labels(wait=True)
    crit = L.BoundaryLoss() if a is None else L.HybirdBoundaryLoss(boundary_weight=a)
    v = crit(x.to(DEV), y.to(DEV))
    with pytest.raises(RuntimeError, match="Class values must be smaller than num_classes."):
        L.raise_on_bad_labels(wait=True)
    assert bool(torch.isnan(v))


def test_argument_errors_on_the_device():
    import _native as N
    y = torch.zeros(1, 4, 4, 4, dtype=torch.int64, device=DEV)
    with pytest.raises(N.Ru3dError, match="three spatial"):
        L.HybirdBoundaryLoss()(torch.zeros(1, 2, 4, 4, device=DEV), torch.zeros(1, 4, 4, dtype=torch.int64, device=DEV))
    with pytest.raises(N.Ru3dError, match="C == 1"):
        L.HybirdBoundaryLoss()(torch.zeros(1, 1, 4, 4, 4, device=DEV), y)
    with pytest.raises(N.Ru3dError, match="classes"):
        L.BoundaryLoss(classes=(1, 1))(torch.zeros(1, 3, 4, 4, 4, device=DEV), y)
    with pytest.raises(N.Ru3dError, match="limit of %d" % N.BOUNDARY_MAX_AXIS):
        L.signed_distance_map(torch.zeros(1, 1, 1, N.BOUNDARY_MAX_AXIS + 1, dtype=torch.uint8, device=DEV), 2)


# ------------------------------------------------------------------------------------------------ captured step
def _batches(n):
    return [(O.synth_image((1, 1, 32, 32, 32), 600 + i).to(DEV), O.phantom_labels(1, (32, 32, 32), 2).to(DEV))
            for i in range(n)]


def _setup():
    torch.manual_seed(5)
    np.random.seed(5)
    ops._drop_counter[0] = 0
    model = network.ResUnet3D(2, 8, 1, 2).to(DEV)
    model.train()
    return model, optim.Adam(model.parameters(), lr=1e-3), L.HybirdBoundaryLoss()


def test_captured_step_equals_eager_and_follows_the_weight():
    """Three steps through GraphedTrainStep leave the eager loop's losses and parameters; set_boundary_weight between
    replays is followed by the next replay, bit for bit, without a recapture; a label out of range raises after a
    replay as it does after an eager step."""
    batches = _batches(5)

    def run(graphed):
        model, opt, crit = _setup()
        step = graph.GraphedTrainStep(model, crit, opt, warmup=1) if graphed else None
        losses, params, seen = [], [], None
        for i, (x, y) in enumerate(batches[:4]):
            if i == 3:
                if graphed:
                    seen = step.graph
                crit.set_boundary_weight(0.05)
                params.append({k: v.clone() for k, v in model.state_dict().items()})
            if graphed:
                losses.append(float(step(x, y)))
            else:
                opt.zero_grad(set_to_none=True)
                v = crit(model(x), y)
                v.backward()
                opt.step()
                losses.append(float(v.detach()))
        torch.cuda.synchronize()
        params.append({k: v.clone() for k, v in model.state_dict().items()})
        assert crit.boundary_weight == 0.05 and float(crit.boundary_weight_buffer) == float(np.float32(0.05))
        if graphed:
            assert step.eager_steps == 1 and step.replays == 3
            assert seen is not None and step.graph is seen          # the graph object was not rebuilt
            # the deferred label check under replay
            L.raise_on_bad_labels(wait=True)
            x, y = batches[4]
            bad = y.clone()
            bad[0, 3, 4, 5] = 2
            v = step(x, bad)
            assert step.graph is seen and step.replays == 4
            with pytest.raises(RuntimeError, match="Class values must be smaller than num_classes."):
                L.raise_on_bad_labels(wait=True)
            assert bool(torch.isnan(v))
            step.release()
        return losses, params

    l_e, p_e = run(False)
    l_g, p_g = run(True)
    assert l_e == l_g, (l_e, l_g)
    assert l_e[3] != l_e[2]
    for when, (pe, pg) in enumerate(zip(p_e, p_g)):
        bad = [k for k in pe if not torch.equal(pe[k], pg[k])]
        assert not bad, (when, bad)


def test_trainer_captures_both_losses_automatically():
    import trainer as T

    class Cases(torch.utils.data.Dataset):
        def __init__(self):
            self.items = [{"image": O.synth_image((1, 1, 32, 32, 32), 600 + i)[0],
                           "label": O.phantom_labels(1, (32, 32, 32), 2)[0]} for i in range(3)]

        def __len__(self):
            return len(self.items)

        def __getitem__(self, i):
            return self.items[i]

    torch.manual_seed(5)
    np.random.seed(5)
    ops._drop_counter[0] = 0
    model = network.ResUnet3D(2, 8, 1, 2).to(DEV)
    tr = T.Trainer(model=model, optimizer=optim.Adam(model.parameters(), lr=1e-3), loss=L.HybirdBoundaryLoss(),
                   dataset=Cases(), batch_size=1, valid_split=0.0, dataloader_kwargs={"num_workers": 0},
                   metrics={"boundary": L.BoundaryLoss()}, progress=False, capture_step=None)
    tr.fit(num_epochs=1)
    torch.cuda.synchronize()
    assert tr.graph_stats["replays"] > 0
