"""CPU-only checks of the soft-clDice feature: the torch twin of the soft skeleton in loss.py (the definition the HIP
kernels are held to) against the published formulation written here with max_pool3d, degenerate extents, binary input
against scipy.ndimage, the lowest-index tie rule of the gradients of E and D against a numpy scatter, the loss algebra
restated in numpy, argument handling, and the names in the header, the bindings and the Makefile."""
import os
import re

import numpy as np
import pytest
import scipy.ndimage as ndi
import torch
import torch.nn.functional as F

import _native as N
import loss as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["ru3d_soft_skeleton_fwd", "ru3d_soft_skeleton_bwd", "ru3d_cldice_workspace_bytes", "ru3d_cldice_fwd",
                "ru3d_cldice_bwd"]


# ------------------------------------------------------------------------------------------------ published formulation
def published_soft_skel(img, iterations):
    """soft_skel of the clDice repository (Shit et al., CVPR 2021), 3D branch, restated."""
    def erode(x):
        p1 = -F.max_pool3d(-x, (3, 1, 1), (1, 1, 1), (1, 0, 0))
        p2 = -F.max_pool3d(-x, (1, 3, 1), (1, 1, 1), (0, 1, 0))
        p3 = -F.max_pool3d(-x, (1, 1, 3), (1, 1, 1), (0, 0, 1))
        return torch.min(torch.min(p1, p2), p3)

    def dilate(x):
        return F.max_pool3d(x, (3, 3, 3), (1, 1, 1), (1, 1, 1))

    def opening(x):
        return dilate(erode(x))

    skel = F.relu(img - opening(img))
    for _ in range(iterations):
        img = erode(img)
        delta = F.relu(img - opening(img))
        skel = skel + F.relu(delta - skel * delta)
    return skel


@pytest.mark.parametrize("k", [0, 1, 3, 5])
def test_twin_is_the_published_formulation_bit_for_bit(k):
    x = torch.rand((2, 2, 12, 10, 9), dtype=torch.float64, generator=torch.Generator().manual_seed(11 + k))
    got = L.soft_skeleton(x, iterations=k)
    assert got.dtype == torch.float64 and got.shape == x.shape
    assert torch.equal(got, published_soft_skel(x, k))


def test_degenerate_extents():
    # a line along Z: E and D see the two line neighbours only
    x = torch.tensor([0.5, 0.9, 0.2, 0.7, 0.8, 0.1, 0.6], dtype=torch.float64)
    # E(x) = [.5 .2 .2 .2 .1 .1 .1], D(E(x)) = [.5 .5 .2 .2 .2 .1 .1]
    got = L.soft_skeleton(x.view(1, 1, 1, 1, 7), iterations=0).view(-1)
    assert got.tolist() == [0.0, 0.9 - 0.5, 0.0, 0.7 - 0.2, 0.8 - 0.2, 0.0, 0.6 - 0.1]
    # two voxels along A: both windows are the whole volume, so E is the minimum, D(E) too, and only the larger survives
    y = torch.tensor([0.25, 0.75], dtype=torch.float64).view(1, 1, 2, 1, 1)
    for k in (0, 1, 3):
        assert L.soft_skeleton(y, iterations=k).view(-1).tolist() == [0.0, 0.5]


def test_binary_input_is_mask_minus_opening():
    rng = np.random.RandomState(5)
    g = ndi.binary_dilation(rng.rand(2, 2, 12, 10, 9) < 0.04, structure=np.ones((1, 1, 3, 3, 3), bool), iterations=1)
    g[0, 0, :, :, 0] = True           # something at a face: the clipping matters
    cross = ndi.generate_binary_structure(3, 1)[None, None]
    cube = np.ones((1, 1, 3, 3, 3), bool)
    er = ndi.binary_erosion(g, structure=cross, border_value=1)     # outside never lowers a minimum
    op = ndi.binary_dilation(er, structure=cube, border_value=0)    # outside never raises a maximum
    want = g & ~op
    got = L.soft_skeleton(torch.from_numpy(g.astype(np.float32)), iterations=0)
    assert got.dtype == torch.float32
    assert np.array_equal(got.numpy(), want.astype(np.float32))
    assert want.any() and not want.all()


# ------------------------------------------------------------------------------------------------ tie rule
E_OFFS = [(-1, 0, 0), (0, -1, 0), (0, 0, -1), (0, 0, 0), (0, 0, 1), (0, 1, 0), (1, 0, 0)]
D_OFFS = [(da, db, dz) for da in (-1, 0, 1) for db in (-1, 0, 1) for dz in (-1, 0, 1)]


def scatter_lowest_index(x, gy, offs, sign):
    """dx of y = min (sign = 1) / max (sign = -1) over the clipped window: each window's gradient goes to the extremal
    candidate with the lowest linear index (candidates are visited in ascending linear index; strict comparison)."""
    a_, b_, z_ = x.shape
    dx = np.zeros_like(x)
    for a in range(a_):
        for b in range(b_):
            for z in range(z_):
                best, at = None, None
                for da, db, dz in offs:
                    p = (a + da, b + db, z + dz)
                    if not (0 <= p[0] < a_ and 0 <= p[1] < b_ and 0 <= p[2] < z_):
                        continue
                    if best is None or sign * x[p] < sign * best:
                        best, at = x[p], p
                dx[at] += gy[a, b, z]
    return dx


def tie_volumes():
    const = np.full((5, 4, 6), 0.5)
    rng = np.random.RandomState(3)
    plateau = np.where(rng.rand(6, 5, 7) < 0.5, 0.25, 0.75)
    return [("constant", const), ("two-level", plateau)]


@pytest.mark.parametrize("name,vol", tie_volumes())
@pytest.mark.parametrize("op", ["E", "D"])
def test_tie_rule_of_the_gradient(name, vol, op):
    offs, sign, fn = (E_OFFS, 1.0, L.soft_erode) if op == "E" else (D_OFFS, -1.0, L.soft_dilate)
    gy = np.random.RandomState(17).randn(*vol.shape)
    x = torch.from_numpy(vol).view((1, 1) + vol.shape).requires_grad_(True)
    y = fn(x)
    y.backward(torch.from_numpy(gy).view_as(y))
    want = scatter_lowest_index(vol, gy, offs, sign)
    got = x.grad.view(vol.shape).numpy()
    assert np.allclose(got, want, rtol=0, atol=1e-12), "%s of %s" % (op, name)
    assert abs(got.sum() - gy.sum()) <= 1e-9
    # every window hands its gradient to exactly one voxel: the value is the extremum
    ref = (ndi.minimum_filter if op == "E" else ndi.maximum_filter)(
        vol, footprint=ndi.generate_binary_structure(3, 1) if op == "E" else np.ones((3, 3, 3), bool), mode="nearest")
    assert np.array_equal(y.detach().view(vol.shape).numpy(), ref)


# ------------------------------------------------------------------------------------------------ loss algebra
def numpy_cldice(logits, labels, k, classes, weight_v, smooth):
    c = logits.shape[1]
    p = torch.softmax(logits, dim=1)
    g = F.one_hot(labels, c).movedim(-1, 1).to(logits.dtype)
    sp = L.soft_skeleton(p, iterations=k).numpy()
    sg = L.soft_skeleton(g, iterations=k).numpy()
    p, g = p.numpy(), g.numpy()
    cls = list(range(1, c)) if classes is None else list(classes)
    w = np.array([1.0 if weight_v is None else weight_v[q] for q in cls], dtype=np.float64)
    w = w / np.abs(w).sum()
    total = 0.0
    for wi, q in zip(w, cls):
        tprec = ((sp[:, q] * g[:, q]).sum() + smooth) / (sp[:, q].sum() + smooth)
        tsens = ((sg[:, q] * p[:, q]).sum() + smooth) / (sg[:, q].sum() + smooth)
        total += wi * (1.0 - 2.0 * tprec * tsens / (tprec + tsens))
    return total


@pytest.mark.parametrize("classes,weight_v,smooth,k", [(None, None, 1.0, 3), ((2,), None, 1.0, 1),
                                                       ((0, 2), [0.2, 0.5, 3.0], 0.25, 2), (None, [1.0, 2.0, 0.5], 1e-3, 0)])
def test_loss_algebra(classes, weight_v, smooth, k):
    gen = torch.Generator().manual_seed(23)
    logits = torch.randn((2, 3, 8, 7, 6), dtype=torch.float64, generator=gen) * 2
    labels = torch.randint(0, 3, (2, 8, 7, 6), generator=gen)
    got = L.SoftClDiceLoss(iterations=k, weight_v=weight_v, classes=classes, smooth=smooth)(logits, labels)
    assert got.dim() == 0 and got.dtype == torch.float64
    want = numpy_cldice(logits, labels, k, classes, weight_v, smooth)
    assert abs(float(got) - want) <= 1e-12 * max(1.0, abs(want))
    assert 0.0 < float(got) < 1.0


def test_label_skeleton_carries_no_gradient_and_loss_is_differentiable():
    gen = torch.Generator().manual_seed(29)
    logits = torch.randn((1, 2, 6, 5, 7), dtype=torch.float64, generator=gen).requires_grad_(True)
    labels = torch.randint(0, 2, (1, 6, 5, 7), generator=gen)
    L.SoftClDiceLoss(iterations=2)(logits, labels).backward()
    assert bool(torch.isfinite(logits.grad).all()) and float(logits.grad.abs().max()) > 0
    # softmax: the gradient over the classes of a voxel sums to zero
    assert float(logits.grad.sum(1).abs().max()) <= 1e-15


# ------------------------------------------------------------------------------------------------ arguments, names
def test_argument_errors():
    with pytest.raises(N.Ru3dError, match="three spatial"):
        L.soft_skeleton(torch.zeros(1, 1, 4, 4))
    with pytest.raises(N.Ru3dError, match="iterations"):
        L.soft_skeleton(torch.zeros(1, 1, 4, 4, 4), iterations=65)
    with pytest.raises(N.Ru3dError, match="iterations"):
        L.HybirdClDiceLoss(iterations=65)
    with pytest.raises(N.Ru3dError, match="three spatial"):
        L.SoftClDiceLoss()(torch.zeros(1, 2, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64))
    with pytest.raises(N.Ru3dError, match="C == 1"):
        L.SoftClDiceLoss()(torch.zeros(1, 1, 4, 4, 4), torch.zeros(1, 4, 4, 4, dtype=torch.int64))
    with pytest.raises(N.Ru3dError, match="classes"):
        L.SoftClDiceLoss(classes=(3,))(torch.zeros(1, 3, 4, 4, 4), torch.zeros(1, 4, 4, 4, dtype=torch.int64))
    assert issubclass(L.SoftClDiceLoss, L._FusedLoss) and issubclass(L.HybirdClDiceLoss, L._FusedLoss)


def test_names_in_header_bindings_and_makefile():
    header = open(os.path.join(ROOT, "include", "ru3d.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in N.SIGNATURES and hasattr(N.lib, name), name
    pkg = os.path.dirname(os.path.abspath(N.__file__))
    assert "cldice.hip" in open(os.path.join(pkg, "csrc", "Makefile")).read()
    # the documented layout: six planes forward (P, G, two x, two s of the label chain), at least two planes gx backward
    plane = 4 * 1080 * 4
    assert N.lib.ru3d_cldice_workspace_bytes(4, 12, 10, 9, 3) >= 6 * plane
    assert N.lib.ru3d_cldice_workspace_bytes(4, 12, 10, 9, 64) >= 6 * plane
    assert N.lib.ru3d_cldice_workspace_bytes(0, 12, 10, 9, 3) == 0
