"""The top-k cross-entropy losses on the host: the torch twin loss._topk_loss_host against an independent float64
definition (F.cross_entropy(reduction='none'), torch.topk(...).values.mean(), autograd through torch.topk's gather), the
K rule, the tie rule on logits built to tie, the argument checks of the classes and of the C entry points (answered before
any launch) and the presence of the new names.  No GPU."""
import ctypes
import os

import pytest
import torch
import torch.nn.functional as F

import _native as N
import loss as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["ru3d_topk_select_workspace_bytes", "ru3d_topk_select", "ru3d_topk_loss_state_bytes",
                "ru3d_topk_loss_workspace_bytes", "ru3d_topk_loss_fwd", "ru3d_topk_loss_bwd"]


def draw(c, shape, seed, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    x = (3 * torch.randn((shape[0], c) + tuple(shape[1:]), generator=g)).to(dtype)
    y = torch.randint(0, c, tuple(shape), generator=g)
    return x, y


def independent(x, y, k):
    """value, gradient, E: torch's own cross-entropy and top-k in float64."""
    z = x.detach().double().requires_grad_(True)
    ce = F.cross_entropy(z, y, reduction="none").reshape(-1)
    kk = max(1, int(ce.numel() * k / 100))
    top = torch.topk(ce, kk).values
    v = top.mean()
    v.backward()
    return float(v.detach()), z.grad, int((ce.detach() == top[-1].detach()).sum())


def twin(x, y, k, **kw):
    z = x.detach().clone().requires_grad_(True)
    v = L._topk_loss_host(z, y, k, **kw)
    v.backward()
    return v.detach(), z.grad


# --------------------------------------------------------------------------- the twin against torch's own ops
@pytest.mark.parametrize("c", [2, 3, 8])
@pytest.mark.parametrize("k", [0.5, 10, 50, 100])
def test_twin_equals_the_independent_definition(c, k):
    x, y = draw(c, (2, 5, 6, 7), seed=100 * c + int(k))
    ref_v, ref_g, e = independent(x, y, k)
    assert e == 1                                      # continuous draws: no ties, torch.topk's gradient is THE gradient
    v, g = twin(x, y, k)
    assert v.dtype == torch.float64
    assert abs(float(v) - ref_v) <= 1e-13 * max(1.0, abs(ref_v))
    assert float((g - ref_g).abs().max()) <= 1e-13 * float(ref_g.abs().max())
    # the module on host tensors is the twin
    z = x.clone().requires_grad_(True)
    m = L.TopKLoss(k=k)(z, y)
    m.backward()
    assert float(m.detach()) == float(v) and torch.equal(z.grad, g)


@pytest.mark.parametrize("c", [2, 5])
def test_k_100_is_the_mean_cross_entropy(c):
    x, y = draw(c, (2, 4, 5, 3), seed=7 + c)
    z = x.clone().requires_grad_(True)
    ref = F.cross_entropy(z, y)
    ref.backward()
    ref = ref.detach()
    v, g = twin(x, y, 100)
    assert abs(float(v) - float(ref)) <= 1e-14 * max(1.0, abs(float(ref)))
    assert float((g - z.grad).abs().max()) <= 1e-14 * float(z.grad.abs().max())


@pytest.mark.parametrize("voxels,k,want", [(1, 10, 1), (7, 10, 1), (9, 10, 1), (10, 10, 1), (19, 10, 1), (20, 10, 2),
                                           (20, 0.5, 1), (200, 0.5, 1), (399, 0.5, 1), (400, 0.5, 2), (7, 100, 7),
                                           (7, 99.9, 6), (3, 50, 1), (2 * 128 ** 3, 10, 419430)])
def test_k_rule(voxels, k, want):
    assert L.topk_count(voxels, k) == want == max(1, int(voxels * k / 100))


@pytest.mark.parametrize("voxels,k", [(1, 10), (3, 10), (7, 10), (7, 50), (2, 100)])
def test_tiny_batches(voxels, k):
    x, y = draw(3, (1, voxels), seed=voxels)
    ref_v, ref_g, e = independent(x, y, k)
    v, g = twin(x, y, k)
    assert e == 1
    assert abs(float(v) - ref_v) <= 1e-13 * max(1.0, abs(ref_v))
    assert float((g - ref_g).abs().max()) <= 1e-13 * float(ref_g.abs().max())
    kk = L.topk_count(voxels, k)
    assert int((g.abs().sum(1) > 0).sum()) == kk       # exactly K voxels carry a gradient


# --------------------------------------------------------------------------- the tie rule
def tie_case(dtype=torch.float64):
    """(2, 2, 10) logits, 20 voxels, k = 25 -> K = 5: three voxels above the threshold (G = 3), exactly four voxels tied at
    it (E = 4, equal logits -> equal ce bits), thirteen below, so K - G = 2 and a tied voxel gets half weight.  Returns
    x, y and the flat positions of the three groups."""
    margins = [-2.0, -3.0, -4.0] + [0.5] * 4 + [1.0 + 0.125 * i for i in range(13)]
    order = torch.randperm(20, generator=torch.Generator().manual_seed(3))
    m = torch.tensor(margins, dtype=dtype)[order]
    y = (torch.arange(20) % 2)[order].reshape(2, 10)
    x = torch.zeros(2, 2, 10, dtype=dtype)
    flat_y = y.reshape(-1)
    xv = torch.zeros(20, 2, dtype=dtype)
    xv[torch.arange(20), flat_y] = m                   # the target logit sits `margin` above the other one (0)
    x[:, 0], x[:, 1] = xv[:, 0].reshape(2, 10), xv[:, 1].reshape(2, 10)
    src = order.tolist()
    above = [i for i, s in enumerate(src) if s < 3]
    tied = [i for i, s in enumerate(src) if 3 <= s < 7]
    below = [i for i, s in enumerate(src) if s >= 7]
    return x, y, above, tied, below


def test_tied_voxels_share_the_remaining_weight():
    x, y, above, tied, below = tie_case()
    v, g = twin(x, y, 25)
    ce = F.cross_entropy(x, y, reduction="none").reshape(-1)
    top = torch.topk(ce, 5).values
    assert int((ce == top[-1]).sum()) == 4 and int((ce > top[-1]).sum()) == 3
    assert abs(float(v) - float(top.mean())) <= 1e-15 * float(top.mean())       # the value is torch.topk's mean
    p = torch.softmax(x, 1).movedim(1, -1).reshape(-1, 2)
    onehot = F.one_hot(y.reshape(-1), 2).double()
    full = (p - onehot) / 5                            # the gradient of a voxel with weight 1
    gv = g.movedim(1, -1).reshape(-1, 2)
    assert torch.allclose(gv[above], full[above], rtol=1e-14, atol=0)
    assert torch.allclose(gv[tied], 0.5 * full[tied], rtol=1e-14, atol=0)      # (K - G) / E = 2 / 4
    assert bool((gv[below] == 0).all())
    labels = y.reshape(-1).tolist()
    for i in tied:                                     # tied voxels with one label: equal logits, equal gradient bits
        for j in tied:
            assert labels[i] != labels[j] or torch.equal(gv[i], gv[j])
    assert sorted(labels[i] for i in tied) == [0, 0, 1, 1]


def test_permuting_the_voxels_permutes_the_gradient_and_nothing_else():
    x, y, *_ = tie_case()
    v, g = twin(x, y, 25)
    perm = torch.randperm(20, generator=torch.Generator().manual_seed(11))
    xp = x.movedim(1, -1).reshape(20, 2)[perm].reshape(2, 10, 2).movedim(-1, 1).contiguous()
    yp = y.reshape(-1)[perm].reshape(2, 10)
    vp, gp = twin(xp, yp, 25)
    assert abs(float(vp) - float(v)) <= 1e-15 * float(v)
    assert torch.equal(gp.movedim(1, -1).reshape(20, 2), g.movedim(1, -1).reshape(20, 2)[perm])


# --------------------------------------------------------------------------- HybirdTopKLoss
@pytest.mark.parametrize("kw", [{}, {"weight_v": [0.2, 1.0, 3.0], "alpha": 0.3, "beta": 0.7, "smooth": 1e-5, "ce_weight": 0.25}])
def test_hybird_topk_on_host_tensors_is_dice_loss_plus_topk(kw):
    x, y = draw(3, (2, 4, 5, 6), seed=21)
    z = x.clone().requires_grad_(True)
    v = L.HybirdTopKLoss(k=10, **kw)(z, y)
    v.backward()
    z2 = x.clone().requires_grad_(True)
    p = torch.softmax(z2, 1)
    g = F.one_hot(y, 3).movedim(-1, 1).double()
    dims = (0, 2, 3, 4)
    tp, sp, sg = (p * g).sum(dims), p.sum(dims), g.sum(dims)
    a, b, s = kw.get("alpha", 0.5), kw.get("beta", 0.5), kw.get("smooth", 1e-7)
    w = torch.tensor(kw.get("weight_v", [1.0, 1.0, 1.0]), dtype=torch.float64)
    w = w / w.abs().sum()
    dice = (tp + s) / (tp + a * (sg - tp) + b * (sp - tp) + s)
    ce = F.cross_entropy(z2, y, reduction="none").reshape(-1)
    ref = (w * (1 - dice)).sum() + kw.get("ce_weight", 1.0) * torch.topk(ce, L.topk_count(ce.numel(), 10)).values.mean()
    ref.backward()
    v, ref = v.detach(), ref.detach()
    assert abs(float(v) - float(ref)) <= 1e-13 * max(1.0, abs(float(ref)))
    assert float((z.grad - z2.grad).abs().max()) <= 1e-13 * float(z2.grad.abs().max())
    # and it is DiceLoss's own host formula plus the twin
    parts = L._region_loss_host(N.LOSS_DICELOSS, x, y, 2.0, kw.get("weight_v"), a, b, s) \
        + kw.get("ce_weight", 1.0) * L._topk_loss_host(x, y, 10)
    assert abs(float(v) - float(parts)) <= 1e-15 * max(1.0, abs(float(parts)))


def test_float32_host_tensors_stay_float32():
    x, y = draw(3, (2, 33), seed=5, dtype=torch.float32)
    v = L.HybirdTopKLoss()(x, y)
    assert v.dtype == torch.float32 and bool(torch.isfinite(v))


# --------------------------------------------------------------------------- argument errors
@pytest.mark.parametrize("k", [0, -1, 100.5, float("nan"), float("inf")])
def test_k_outside_the_range_is_refused(k):
    for cls in (L.TopKLoss, L.HybirdTopKLoss):
        with pytest.raises(ValueError):
            cls(k=k)
    x, y = draw(2, (1, 9), seed=1)
    with pytest.raises(ValueError):
        L._topk_loss_host(x, y, k)


def test_argument_errors_of_a_call():
    L.TopKLoss(k=100), L.TopKLoss(k=0.001), L.HybirdTopKLoss(k=1e-9)
    x, y = draw(3, (1, 9), seed=2)
    with pytest.raises(ValueError, match="C == 1"):
        L.TopKLoss()(x[:, :1], torch.zeros_like(y))
    with pytest.raises(ValueError, match="C == 1"):
        L.HybirdTopKLoss()(x[:, :1], torch.zeros_like(y))
    with pytest.raises(ValueError, match="weight_v"):
        L.HybirdTopKLoss(weight_v=[1.0, 2.0])(x, y)
    with pytest.raises(RuntimeError, match="Class values must be smaller than num_classes."):
        L.TopKLoss()(x, y + 1)
    with pytest.raises(N.Ru3dError, match="target shape"):
        L.TopKLoss()(x, y[:, :8])


def test_deep_supervision_keeps_refusing_a_topk_base():
    with pytest.raises(TypeError):
        L.DeepSupervisionLoss(L.HybirdTopKLoss())
    with pytest.raises(TypeError):
        L.DeepSupervisionLoss(L.TopKLoss())


def test_the_losses_are_fused_losses():
    assert issubclass(L.TopKLoss, L._FusedLoss) and issubclass(L.HybirdTopKLoss, L._FusedLoss)
    assert "recapture" in L.TopKLoss.__doc__ and "recapture" in L.HybirdTopKLoss.__doc__


# --------------------------------------------------------------------------- the C ABI, before any launch
def test_entry_points_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "ru3d.h")).read()
    for name in ENTRY_POINTS:
        assert name + "(" in header and name in N.SIGNATURES and hasattr(N.lib, name)
    assert N.lib.ru3d_topk_loss_state_bytes() >= N.lib.ru3d_loss_state_bytes(3) - 8 + 4 + 3 * 8 + 2 * 4
    assert N.lib.ru3d_topk_select_workspace_bytes(1) > 0 and N.lib.ru3d_topk_select_workspace_bytes(0) == 0
    assert N.lib.ru3d_topk_loss_workspace_bytes(2, 1000, 3) > N.lib.ru3d_topk_select_workspace_bytes(2000)


def test_c_abi_refuses_before_launch():
    fake = ctypes.c_void_p(4096)                       # never dereferenced: every call below is refused on its arguments
    sel = N.lib.ru3d_topk_select
    for n, kk, vals, res, ws, nbytes in [(0, 1, fake, fake, fake, 1 << 20), (10, 0, fake, fake, fake, 1 << 20),
                                         (10, 11, fake, fake, fake, 1 << 20), (10, 1, None, fake, fake, 1 << 20),
                                         (10, 1, fake, None, fake, 1 << 20), (10, 1, fake, fake, None, 1 << 20),
                                         (10, 1, fake, fake, fake, 16), (10, 1, ctypes.c_void_p(4098), fake, fake, 1 << 20)]:
        assert sel(vals, n, kk, res, ws, nbytes, None) != 0
        assert N.lib.ru3d_last_error()
    big = 1 << 24

    def fwd(c=3, n=2, v=100, kk=20, label=N.LABEL_I64, ce=fake, ws_bytes=big):
        return N.lib.ru3d_topk_loss_fwd(fake, c * v, v, 1, fake, label, n, v, c, kk, 1, None, 0.5, 0.5, 1e-7, 1.0, ce, fake,
                                        fake, fake, ws_bytes, None)

    assert fwd(c=1) != 0 and fwd(c=9) != 0 and fwd(kk=0) != 0 and fwd(kk=201) != 0 and fwd(label=7) != 0
    assert fwd(ce=None) != 0 and fwd(ws_bytes=64) != 0 and fwd(n=0) != 0

    def bwd(c=3, dt=N.F32, ce=fake):
        return N.lib.ru3d_topk_loss_bwd(fake, c * 100, 100, 1, fake, N.LABEL_U8, 2, 100, c, 1, ce, fake, None, fake, dt, None)

    assert bwd(c=1) != 0 and bwd(dt=99) != 0 and bwd(ce=None) != 0
