"""What every fused loss owes its caller, whatever it computes: all fifteen criteria of loss.py go through one call path
(operands -> forward scaffold -> ABI call(s) -> noted state -> backward scaffold), and the checks
tests/test_gpu_loss_kernels.py makes of the four base kinds are made here of every one of them, on a real MI355X.

Every check compares a criterion with a second run of the same criterion by torch.equal: there is no reference and no
tolerance.  The shapes are the smallest at which the shared code can go wrong: logits (2, 3, 6, 5, 7) - 420 voxels, odd
extents, two samples - with labels (2, 6, 5, 7); deep supervision adds the level (3, 3, 4); the group losses have two
channels over three label values (nested groups); top-k has k = 10, K = 42.

The file uses the public API only, and every check passed unchanged on the commit before the shared path existed: none
had to be narrowed for any criterion.

Above the grid caps (2048 forward blocks, 8192 backward blocks) the flat families - region, groups, top-k - are held to
their host twins.  Region and groups have such a case in their own files
(test_gpu_loss_kernels.py::test_voxel_counts_around_the_reduction_layout[3-1400003],
test_gpu_groups.py::test_voxel_counts_around_the_reduction_layout[4194307] - 2048 * 2048 + 3 voxels); top-k has none, so
it gets one here, with the tolerances of tests/test_gpu_topk.py.
Run with `-m gpu`."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no HIP device", allow_module_level=True)

import loss as L  # noqa: E402

DEV = torch.device("cuda:0")
BAD_LABELS = "Class values must be smaller than num_classes."
NESTED = ((1, 2), (2,))
SPATIAL = (6, 5, 7)
LEVEL1 = (3, 3, 4)

# name -> (factory, channels, deep supervision)
CRITERIA = {
    "Dice": (lambda: L.Dice(), 3, False),
    "DiceLoss": (lambda: L.DiceLoss(), 3, False),
    "FocalLoss": (lambda: L.FocalLoss(), 3, False),
    "HybirdLoss": (lambda: L.HybirdLoss(), 3, False),
    "SoftClDiceLoss": (lambda: L.SoftClDiceLoss(iterations=2), 3, False),
    "HybirdClDiceLoss": (lambda: L.HybirdClDiceLoss(cl_weight=0.5, iterations=2), 3, False),
    "BoundaryLoss": (lambda: L.BoundaryLoss(), 3, False),
    "HybirdBoundaryLoss": (lambda: L.HybirdBoundaryLoss(), 3, False),
    "DeepSupervisionLoss": (lambda: L.DeepSupervisionLoss(L.HybirdLoss()), 3, True),
    "GroupDice": (lambda: L.GroupDice(NESTED), 2, False),
    "GroupDiceLoss": (lambda: L.GroupDiceLoss(NESTED), 2, False),
    "GroupFocalLoss": (lambda: L.GroupFocalLoss(NESTED), 2, False),
    "GroupHybirdLoss": (lambda: L.GroupHybirdLoss(NESTED), 2, False),
    "TopKLoss": (lambda: L.TopKLoss(k=10), 3, False),
    "HybirdTopKLoss": (lambda: L.HybirdTopKLoss(k=10), 3, False),
}
NAMES = list(CRITERIA)


def draw(name, seed=7, extra=(0, 0, 0)):
    """float32 logits of the criterion's levels (a list; one level unless deep supervision) and int64 labels, on the
    device.  extra: voxels added to every spatial axis, for a caller that slices them off again."""
    _, c, ds = CRITERIA[name]
    g = torch.Generator().manual_seed(seed)
    shapes = [SPATIAL, LEVEL1] if ds else [SPATIAL]
    xs = [2.0 * torch.randn((2, c) + tuple(s + e for s, e in zip(shape, extra)), generator=g) for shape in shapes]
    y = torch.randint(0, 3, (2,) + SPATIAL, generator=g)
    return [x.to(DEV) for x in xs], y.to(DEV)


def run(name, xs, y, upstream=None, gradient=None, crit=None):
    """Value and the gradient of every level; the logits keep their strides and their dtype."""
    crit = CRITERIA[name][0]() if crit is None else crit
    xs = [x.detach().requires_grad_(True) for x in xs]
    v = crit(xs if CRITERIA[name][2] else xs[0], y)
    assert v.dim() == 0 and v.is_cuda and v.dtype == torch.float32
    (v if upstream is None else upstream(v)).backward(gradient)
    for x in xs:
        assert x.grad.shape == x.shape and x.grad.dtype == x.dtype
    return v.detach(), [x.grad.detach() for x in xs]


def same(a, b):
    (va, ga), (vb, gb) = a, b
    return torch.equal(va, vb) and len(ga) == len(gb) and all(torch.equal(p, q) for p, q in zip(ga, gb))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("name", NAMES)
def test_sixteen_bit_logits_are_their_float32_values(name, dtype):
    xs, y = draw(name)
    x16 = [x.to(dtype) for x in xs]
    v32, g32 = run(name, [x.float() for x in x16], y)
    v16, g16 = run(name, x16, y)
    assert torch.equal(v16, v32)
    for a, b in zip(g16, g32):
        assert torch.equal(a, b.to(dtype))


@pytest.mark.parametrize("name", NAMES)
def test_strides_do_not_change_a_bit(name):
    big, y = draw(name, extra=(0, 2, 3))
    xs = [b[:, :, :, 1:-1, 2:-1] for b in big]                     # spatial strides that do not collapse
    assert all(L._flat_strides(x) is None for x in xs)
    dense = run(name, [x.contiguous() for x in xs], y)
    assert same(run(name, xs, y), dense)
    last = [x.contiguous(memory_format=torch.channels_last_3d) for x in xs]
    assert all(x.stride(1) == 1 for x in last)
    assert same(run(name, last, y), dense)


@pytest.mark.parametrize("name", NAMES)
def test_label_types(name):
    xs, y = draw(name)
    first = run(name, xs, y)
    assert same(run(name, xs, y.to(torch.uint8)), first)
    assert same(run(name, xs, y.to(torch.int32)), first)


@pytest.mark.parametrize("name", NAMES)
def test_upstream_gradient_scales_exactly(name):
    xs, y = draw(name)
    v, g1 = run(name, xs, y)
    for factor in (65536.0, 2.0 ** -20, -1.0):                     # powers of two: exact
        _, gs = run(name, xs, y, upstream=lambda t: factor * t)
        for a, b in zip(gs, g1):
            assert torch.equal(a, factor * b), factor
    as32 = run(name, xs, y, gradient=torch.tensor(-1.0, dtype=torch.float32, device=DEV))
    as64 = run(name, xs, y, gradient=torch.tensor(-1.0, dtype=torch.float64, device=DEV))
    assert same(as64, as32)


@pytest.mark.parametrize("name", NAMES)
def test_a_label_out_of_range(name):
    L.raise_on_bad_labels(wait=True)
    xs, y = draw(name)
    bad = y.clone()
    bad[1, 2, 3, 4] = 3
    crit = CRITERIA[name][0]()
    crit.check_labels = False
    v = crit(xs if CRITERIA[name][2] else xs[0], bad)
    with pytest.raises(RuntimeError, match=BAD_LABELS):
        L.raise_on_bad_labels(wait=True)
    assert bool(torch.isnan(v))
    crit.check_labels = True
    with pytest.raises(RuntimeError, match=BAD_LABELS):
        crit(xs if CRITERIA[name][2] else xs[0], bad)
    crit.check_labels = False
    v = crit(xs if CRITERIA[name][2] else xs[0], y)
    L.raise_on_bad_labels(wait=True)
    assert bool(torch.isfinite(v))


@pytest.mark.parametrize("name", NAMES)
def test_same_input_same_bits(name):
    xs, y = draw(name)
    assert same(run(name, xs, y), run(name, xs, y))


# ------------------------------------------------------------------------------------------------ above the grid caps
VALUE_TOL = 2e-6             # tests/test_gpu_topk.py
GRAD_REL = 2e-5
GRAD_FLOOR = 1e-6


@pytest.mark.parametrize("name", ["TopKLoss", "HybirdTopKLoss"])
def test_topk_above_the_grid_caps(name):
    """n = 1, two classes, V = 2048 * 2048 + 2049: beyond 2048 forward blocks of 2048 voxels and beyond 8192 backward
    blocks of 256, against _topk_loss_host in float64 on a host copy.  k = 100: every voxel is selected, so no voxel
    sits near a threshold on which float32 and float64 could disagree, and every gradient element is compared."""
    v = 2048 * 2048 + 2049
    g = torch.Generator().manual_seed(2049)
    x = 3 * torch.randn((1, 2, v), generator=g)
    y = torch.randint(0, 2, (1, v), generator=g)
    z = x.double().requires_grad_(True)
    ref = L._topk_loss_host(z, y, 100, with_dice=name == "HybirdTopKLoss")
    ref.backward()
    ref_v, ref_g = float(ref.detach()), z.grad
    crit = L.TopKLoss(k=100) if name == "TopKLoss" else L.HybirdTopKLoss(k=100)
    dx = x.to(DEV).requires_grad_(True)
    got = crit(dx, y.to(DEV))
    got.backward()
    got_v, got_g = float(got.detach()), dx.grad.detach().to("cpu", torch.float64)
    print("%s: value %.9g, host twin %.9g" % (name, got_v, ref_v))
    assert abs(got_v - ref_v) <= VALUE_TOL * max(1.0, abs(ref_v))
    err = (got_g - ref_g).abs()
    tol = GRAD_REL * ref_g.abs() + GRAD_FLOOR * float(ref_g.abs().max())
    worst = float((err / tol).max())
    print("%s: worst gradient element %.3g of its bound" % (name, worst))
    assert bool(torch.isfinite(got_g).all()) and worst <= 1.0
