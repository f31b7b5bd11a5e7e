"""CPU-only checks of deep supervision: the level weights, the label rule (loss.downsample_labels against
F.interpolate(mode='nearest')), the auxiliary heads' place in the construction order (every reference parameter keeps its
default initialisation), argument handling, the list a training-mode forward returns against the single tensor of eval
mode, the host twin of DeepSupervisionLoss against the formula written out here in float64, the C entry points' argument
checks (which answer before any launch), and the names in the header, the bindings, the library and the Makefile."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

import _native as N
import loss as L
import network

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["ru3d_ds_state_bytes", "ru3d_ds_state_bad_labels_offset", "ru3d_ds_block_bytes",
                "ru3d_ds_loss_workspace_bytes", "ru3d_ds_loss_fwd", "ru3d_ds_loss_bwd"]


# ------------------------------------------------------------------------------------------------ weights, labels
def test_weights_halve_per_level_and_sum_to_one():
    assert L.deep_supervision_weights(3) == [4 / 7, 2 / 7, 1 / 7]
    assert L.deep_supervision_weights(1) == [1.0]
    for levels in range(1, N.DS_MAX_LEVELS + 1):
        ws = L.deep_supervision_weights(levels)
        assert len(ws) == levels and abs(sum(ws) - 1.0) < 1e-15
        assert all(abs(ws[l] - 2 * ws[l + 1]) < 1e-15 for l in range(levels - 1))
    with pytest.raises(ValueError):
        L.deep_supervision_weights(0)
    with pytest.raises(ValueError):
        L.deep_supervision_weights(N.DS_MAX_LEVELS + 1)


def test_label_rule_is_nearest_interpolation():
    g = torch.Generator().manual_seed(3)
    label = torch.randint(0, 4, (2, 20, 12, 10), generator=g)
    assert L.downsample_labels(label, 0) is label or torch.equal(L.downsample_labels(label, 0), label)
    for level, shape in ((1, (10, 6, 5)), (2, (5, 3, 3))):      # 10 -> 5 -> 3: the ceil rule
        got = L.downsample_labels(label, level)
        assert tuple(got.shape) == (2,) + shape
        assert got.data_ptr() == label.data_ptr()      # a view: no copy
        step = 1 << level
        assert torch.equal(got, label[:, ::step, ::step, ::step])
        # F.interpolate(size=...) maps output index i to floor(i * in / out): the step 2**level wherever it divides the
        # extent.  On the one axis where it does not (10 -> 3 at level 2: in / out = 10 / 3, columns 0, 3, 6) the rule
        # label[a << s] (columns 0, 4, 8) is nearest interpolation of the labels padded to a multiple of the step, whose
        # pad voxels are never picked
        plain = F.interpolate(label[:, None].double(), size=shape, mode='nearest')[:, 0]
        divides = [s % step == 0 for s in label.shape[1:]]
        if all(divides):
            assert torch.equal(got.double(), plain)
        else:
            assert level == 2 and divides == [True, True, False]
            assert torch.equal(got.double()[..., 0], plain[..., 0])      # column 0 is column 0 under either scale
        pads = [(-s) % step for s in label.shape[1:]]
        padded = F.pad(label, (0, pads[2], 0, pads[1], 0, pads[0]), value=-1)
        ref = F.interpolate(padded[:, None].double(), size=shape, mode='nearest')[:, 0]
        assert torch.equal(got.double(), ref)


def test_main_output():
    a, b = torch.zeros(2), torch.ones(2)
    assert L.main_output(a) is a
    assert L.main_output([a, b]) is a and L.main_output((a, b)) is a


# ------------------------------------------------------------------------------------------------ network
def test_aux_heads_leave_the_reference_initialisation_alone():
    torch.manual_seed(0)
    plain = network.ResUnet3D(2, 8, 1, 3).state_dict()
    torch.manual_seed(0)
    deep = network.ResUnet3D(2, 8, 1, 3, deep_supervision=2).state_dict()
    assert set(deep) - set(plain) == {"net.ds_heads.0.weight", "net.ds_heads.0.bias"}
    assert set(plain) <= set(deep)
    for k, v in plain.items():
        assert torch.equal(v, deep[k]), k
    assert tuple(deep["net.ds_heads.0.weight"].shape) == (3, 16, 1, 1, 1)      # decoder level 1: 2 * F channels
    # off is off: 0 and 1 give the same keys as the class without the keyword
    for off in (0, 1):
        torch.manual_seed(0)
        sd = network.ResUnet3D(2, 8, 1, 3, deep_supervision=off).state_dict()
        assert list(sd) == list(plain)


def test_argument_checks():
    with pytest.raises(ValueError, match="deep_supervision"):
        network.ResUnet3D(2, 8, 1, 3, deep_supervision=3)
    with pytest.raises(ValueError, match="deep_supervision"):
        network.ResUnet3D(1, 8, 1, 3, deep_supervision=2)
    with pytest.raises(ValueError, match="deep_supervision"):
        network.ResUnet3D(2, 8, 1, 3, deep_supervision=-1)
    for cls in (network.ResAttrUnet3D, network.ResAttrBNUnet3D):
        m = cls(2, 8, 1, 2, deep_supervision=2)
        assert len(m.net.ds_heads) == 1
    assert len(network.ResAttrUnet3D2(1, 2, deep_supervision=5).net.ds_heads) == 4
    with pytest.raises(TypeError, match="HybirdLoss, DiceLoss or FocalLoss"):
        L.DeepSupervisionLoss(L.Dice())
    with pytest.raises(TypeError):
        L.DeepSupervisionLoss(torch.nn.CrossEntropyLoss())
    crit = L.DeepSupervisionLoss(L.HybirdLoss(), weights=[0.5, 0.5])
    x = [torch.zeros(1, 2, 4, 4, 4), torch.zeros(1, 2, 2, 2, 2), torch.zeros(1, 2, 1, 1, 1)]
    y = torch.zeros(1, 4, 4, 4, dtype=torch.int64)
    with pytest.raises(ValueError, match="weights"):
        crit(x, y)
    with pytest.raises(N.Ru3dError, match="level 1"):
        crit([x[0], x[2]], y)
    with pytest.raises(N.Ru3dError, match="target shape"):
        crit(x[:2], y[:, :2])
    assert issubclass(L.DeepSupervisionLoss, L._FusedLoss)      # Trainer's automatic capture takes it


def torch_twin(model):
    """The torch fallback of a native model: every block, the stem and the heads run as the torch modules they are built
    from (the native blocks refuse host tensors; their torch bodies are the reference's), Dropout3d switched off."""
    for m in model.modules():
        if hasattr(m, "_native"):
            m._native = False
        if isinstance(m, torch.nn.Dropout3d):
            m.p = 0.0
    model.net._native_io = False
    model.net._configure_native()
    return model


def test_train_mode_returns_the_list_eval_mode_the_tensor():
    torch.manual_seed(1)
    model = torch_twin(network.ResUnet3D(2, 8, 1, 3, deep_supervision=2))
    assert not model.net._in_chain and not model.net._linked      # torch modules all the way
    x = torch.randn(2, 1, 16, 16, 16, generator=torch.Generator().manual_seed(2))
    model.train()
    out = model(x)
    assert isinstance(out, list) and len(out) == 2
    assert tuple(out[0].shape) == (2, 3, 16, 16, 16) and tuple(out[1].shape) == (2, 3, 8, 8, 8)
    assert all(o.dtype == torch.float32 for o in out)
    # InstanceNorm without running statistics and no dropout: train and eval compute the same function
    model.eval()
    single = model(x)
    assert torch.is_tensor(single) and torch.equal(single, out[0])
    # the aux entry is the aux head on the level's output: its gradient reaches the head and the decoder below it only
    net = model.net
    out[1].sum().backward()
    assert net.ds_heads[0].weight.grad is not None and net.fc.weight.grad is None
    assert net.decode_blocks[1].conv1.weight.grad is not None and net.decode_blocks[0].conv1.weight.grad is None
    # a model built without the keyword returns the tensor in both modes
    plain = torch_twin(network.ResUnet3D(2, 8, 1, 3)).train()
    assert torch.is_tensor(plain(x))


# ------------------------------------------------------------------------------------------------ host twin
def reference_level(kind, z, y, gamma, weight_v, alpha, beta, smooth):
    """One level's loss in float64, the formulas of csrc/loss.hip's header comment written out."""
    n, c = z.shape[0], z.shape[1]
    zf = z.reshape(n, c, -1)
    yf = y.long().reshape(n, 1, -1)
    logp = torch.log_softmax(zf, dim=1)
    p = logp.exp()
    g = torch.zeros_like(zf).scatter_(1, yf, 1.0)
    w = torch.tensor([1.0] * c if weight_v is None else weight_v, dtype=torch.float64)
    w = w / w.abs().sum()
    tp, sp, sg = (p * g).sum((0, 2)), p.sum((0, 2)), g.sum((0, 2))
    dice = (tp + smooth) / (tp + alpha * (sg - tp) + beta * (sp - tp) + smooth)
    focal = (-((1.0 - p) ** gamma) * g * logp).sum((0, 2)) * c / (n * zf.shape[2])
    if kind == "HybirdLoss":
        return (w * (1.0 - dice + focal)).sum()
    if kind == "DiceLoss":
        return (w * (1.0 - dice)).sum()
    return (w * focal).sum()


@pytest.mark.parametrize("kind", ["HybirdLoss", "DiceLoss", "FocalLoss"])
def test_host_twin_matches_the_formula(kind):
    g = torch.Generator().manual_seed(11)
    shapes = [(20, 12, 10), (10, 6, 5), (5, 3, 3)]
    outs = [torch.randn((2, 3) + s, generator=g, dtype=torch.float64).requires_grad_(True) for s in shapes]
    y = torch.randint(0, 3, (2, 20, 12, 10), generator=g)
    wv = [0.2, 0.3, 0.5]
    if kind == "HybirdLoss":
        base, hyper = L.HybirdLoss(gamma=2, weight_v=wv, alpha=0.3, beta=0.7, smooth=1e-5), (2, wv, 0.3, 0.7, 1e-5)
    elif kind == "DiceLoss":
        base, hyper = L.DiceLoss(weight_v=wv, alpha=0.3, beta=0.7, smooth=1e-5), (2, wv, 0.3, 0.7, 1e-5)
    else:
        base, hyper = L.FocalLoss(gamma=1.5, weight_v=wv), (1.5, wv, 0.5, 0.5, 1e-7)
    crit = L.DeepSupervisionLoss(base)
    got = crit(outs, y)
    ws = L.deep_supervision_weights(3)
    refs = [reference_level(kind, o, L.downsample_labels(y, l), *hyper) for l, o in enumerate(outs)]
    ref = sum(w * r for w, r in zip(ws, refs))
    assert got.dtype == torch.float64 and abs(float(got.detach()) - float(ref.detach())) <= 1e-12 * max(1.0, abs(float(ref.detach())))
    assert torch.allclose(crit.last_level_losses.double(), torch.stack(refs).detach(), rtol=1e-6, atol=1e-7)
    got_g = torch.autograd.grad(got, outs)
    ref_g = torch.autograd.grad(ref, outs)
    for a, b in zip(got_g, ref_g):
        assert torch.allclose(a, b, rtol=1e-9, atol=1e-14)
    # explicit weights, set_weights, and the single tensor (one level, weight 1: the base loss itself)
    crit.set_weights([0.5, 0.25, 0.25])
    assert crit.weights == [0.5, 0.25, 0.25]
    got2 = crit(outs, y)
    ref2 = 0.5 * refs[0] + 0.25 * refs[1] + 0.25 * refs[2]
    assert abs(float(got2.detach()) - float(ref2.detach())) <= 1e-12 * max(1.0, abs(float(ref2.detach())))
    one = crit(outs[0], y)
    assert abs(float(one.detach()) - float(refs[0].detach())) <= 1e-12 * max(1.0, abs(float(refs[0].detach())))
    with pytest.raises(RuntimeError, match="Class values must be smaller than num_classes"):
        crit(outs, torch.full_like(y, 3))


# ------------------------------------------------------------------------------------------------ C ABI
def test_names_in_header_bindings_and_makefile():
    header = open(os.path.join(ROOT, "include", "ru3d.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in N.SIGNATURES and hasattr(N.lib, name), name
    pkg = os.path.dirname(os.path.abspath(N.__file__))
    assert "deepsup.hip" in open(os.path.join(pkg, "csrc", "Makefile")).read()
    assert re.search(r"#define\s+RU3D_DS_MAX_LEVELS\s+%d\b" % N.DS_MAX_LEVELS, header)
    assert N.lib.ru3d_ds_block_bytes() == 4 * (2 * N.DS_MAX_LEVELS + 1)
    # level 0's count of out-of-range labels sits where every fused loss keeps it
    assert N.lib.ru3d_ds_state_bad_labels_offset() == N.lib.ru3d_loss_state_bad_labels_offset()
    assert N.lib.ru3d_ds_state_bytes() > N.lib.ru3d_ds_state_bad_labels_offset() + 4
    assert ctypes.sizeof(N.DsLevel) == 48


def _table(shapes, shifts, base=0x1000):
    t = (N.DsLevel * len(shapes))()
    for l, ((d, h, w), s) in enumerate(zip(shapes, shifts)):
        t[l] = N.DsLevel(base, d * h * w * 3, d * h * w, 1, d, h, w, s)
    return t


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """Every call below must return an error from the argument checks: no HIP device is touched (the pointers are fakes)."""
    fake = ctypes.c_void_p(0x1000)
    good = _table([(20, 12, 10), (10, 6, 5), (5, 3, 3)], [0, 1, 2])
    # one row of 33 doubles per block: ceil(2 * v / 2048) blocks per level
    assert N.lib.ru3d_ds_loss_workspace_bytes(good, 3, 2) == (3 + 1 + 1) * 33 * 8
    assert N.lib.ru3d_ds_loss_workspace_bytes(good, 0, 2) == 0
    assert N.lib.ru3d_ds_loss_workspace_bytes(good, N.DS_MAX_LEVELS + 1, 2) == 0

    def fwd(table, levels, extents=(20, 12, 10), c=3, kind=N.LOSS_HYBIRD, lab=N.LABEL_I64, ws_bytes=1 << 20):
        return N.lib.ru3d_ds_loss_fwd(table, levels, fake, lab, 2, extents[0], extents[1], extents[2], c, kind, 2.0, None,
                                      0.5, 0.5, 1e-7, fake, fake, fake, fake, ws_bytes, None)

    def refused(rc, text):
        assert rc != 0
        msg = N.lib.ru3d_last_error().decode()
        assert text in msg, msg

    refused(fwd(good, 0), "levels")
    refused(fwd(good, N.DS_MAX_LEVELS + 1), "levels")
    refused(fwd(good, 3, c=9), "classes")
    refused(fwd(good, 3, kind=N.LOSS_DICE), "kind")
    refused(fwd(good, 3, lab=7), "label dtype")
    refused(fwd(good, 3, ws_bytes=8), "workspace too small")
    # a level that would read labels outside the tensor: 11 rows at shift 1 reach row 20 of 20
    refused(fwd(_table([(20, 12, 10), (11, 6, 5)], [0, 1]), 2), "reaches outside")
    refused(fwd(_table([(20, 12, 10), (10, 6, 6)], [0, 1]), 2), "reaches outside")
    refused(fwd(_table([(20, 12, 10), (10, 6, 5)], [0, 2]), 2), "reaches outside")
    refused(fwd(_table([(10, 6, 5)], [1]), 1), "level 0")
    refused(fwd(_table([(20, 12, 10), (10, 6, 5)], [0, -1]), 2), "shift")
    refused(fwd(_table([(20, 12, 10)], [0], base=0), 1), "no logits")
    none = (ctypes.c_void_p * 2)(0x1000, None)
    rc = N.lib.ru3d_ds_loss_bwd(_table([(20, 12, 10), (10, 6, 5)], [0, 1]), none, 2, fake, N.LABEL_U8, 2, 20, 12, 10, 3, 2.0,
                                fake, None, None)
    refused(rc, "no dlogits")
