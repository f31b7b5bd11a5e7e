"""Overlapping label groups on the host: the membership table, the numpy twins of transform.py, the torch twin of the four
group losses against the formulas written out here in float64, evaluate_groups_case on numpy volumes, the argument checks
of the C entry points (answered before any launch) and the presence of the new names.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _native as N
import loss as L
import trainer as T
import transform as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["ru3d_group_loss_state_bytes", "ru3d_group_loss_workspace_bytes", "ru3d_group_loss_fwd",
                "ru3d_group_loss_bwd", "ru3d_predict_accumulate_groups", "ru3d_predict_merge_groups"]
KINDS = ["GroupHybirdLoss", "GroupDiceLoss", "GroupFocalLoss", "GroupDice"]
NESTED = ((1, 2), (2,))


# --------------------------------------------------------------------------- group_table
def test_group_table_bytes():
    assert L.group_table(NESTED) == bytes([0, 1, 3])
    assert L.group_table(NESTED, num_labels=5) == bytes([0, 1, 3, 0, 0])
    assert L.group_table(((1,), (2,), (3,))) == bytes([0, 1, 2, 4])
    assert L.group_table(((0, 3), (3,), (1,))) == bytes([1, 4, 0, 3])
    assert L.group_table([[31]]) == bytes([0] * 31 + [1])
    assert L.group_table(tuple((k + 1,) for k in range(8))) == bytes([0] + [1 << k for k in range(8)])


@pytest.mark.parametrize("groups,kw", [
    ((), {}),                                                 # K = 0
    (tuple((k + 1,) for k in range(9)), {}),                  # K = 9
    (((1, 32),), {}),                                         # a value of 32
    (((1, 2),), {"num_labels": 2}),                           # a value outside [0, T)
    (((1,),), {"num_labels": 33}),                            # T = 33
    (((1, 2), ()), {}),                                       # an empty group
    (((1, 2, 1),), {}),                                       # a repeated value
    (((1, 2), (2, 1)), {}),                                   # two groups equal as sets
    (((-1, 2),), {}),                                         # a negative value
], ids=["k0", "k9", "value32", "outside", "t33", "empty", "repeated", "equal", "negative"])
def test_group_table_refuses(groups, kw):
    with pytest.raises(ValueError):
        L.group_table(groups, **kw)
    with pytest.raises(ValueError):
        L.GroupHybirdLoss(groups, **kw)


@pytest.mark.parametrize("ignore", [0, 1, 2])
def test_ignore_label_inside_the_label_range_is_refused(ignore):
    for cls in (L.GroupDice, L.GroupDiceLoss, L.GroupFocalLoss, L.GroupHybirdLoss):
        with pytest.raises(ValueError):
            cls(NESTED, ignore_label=ignore)
    L.GroupHybirdLoss(NESTED, ignore_label=3)
    L.GroupHybirdLoss(NESTED, ignore_label=-1)
    with pytest.raises(ValueError):
        L.GroupHybirdLoss(NESTED, num_labels=4, ignore_label=3)


# --------------------------------------------------------------------------- numpy twins
def test_labels_to_groups_equals_the_loop():
    rng = np.random.RandomState(3)
    label = rng.randint(0, 6, size=(2, 4, 5, 6))
    groups = ((1, 2, 5), (2,), (0, 4), (5, 3))
    got = TR.labels_to_groups(label, groups)
    assert got.dtype == np.uint8 and got.shape == (4,) + label.shape
    want = np.zeros_like(got)
    for idx in np.ndindex(*label.shape):
        for k, g in enumerate(groups):
            want[(k,) + idx] = 1 if int(label[idx]) in g else 0
    assert np.array_equal(got, want)
    # num_labels below a label that occurs: that label is a member of nothing
    wide = TR.labels_to_groups(np.array([0, 1, 2, 7, 255], dtype=np.uint8), NESTED)
    assert wide.tolist() == [[0, 1, 1, 0, 0], [0, 0, 1, 0, 0]]


def test_default_group_labels():
    assert TR.default_group_labels(((1, 2), (2,))) == (1, 2)
    assert TR.default_group_labels(((1, 2), (2,), (3,))) == (1, 2, 3)
    assert TR.default_group_labels(((2,), (1, 2))) == (2, 1)
    assert TR.default_group_labels(((1,), (1, 2), (1, 2, 3))) == (1, 2, 3)
    with pytest.raises(ValueError):
        TR.default_group_labels(((1, 2), (1,), (2,)))
    with pytest.raises(ValueError):
        TR.groups_to_labels(np.zeros((3, 3), dtype=np.float32), ((1, 2), (1,), (2,)))
    got = TR.groups_to_labels(np.ones((2, 3), dtype=bool), ((1, 2), (1,), (2,)), group_labels=(3, 1, 2))
    assert got.tolist() == [2, 2]


def test_groups_to_labels_rule():
    nan = float("nan")
    q = np.array([[0.9, 0.8],         # both on: the later group wins
                  [0.9, 0.1],         # the first alone
                  [0.1, 0.9],         # the later alone
                  [0.2, 0.3],         # nothing on
                  [nan, nan],         # NaN is off
                  [0.9, nan],
                  [0.5, 0.5],         # exactly at the threshold: off
                  [np.nextafter(np.float32(0.5), np.float32(1)), 0.5]], dtype=np.float32)
    assert TR.groups_to_labels(q, NESTED).tolist() == [2, 1, 2, 0, 0, 1, 0, 1]
    assert TR.groups_to_labels(q, NESTED).dtype == np.uint8
    assert TR.groups_to_labels(q, NESTED, group_labels=(7, 9)).tolist() == [9, 7, 9, 0, 0, 7, 0, 7]
    assert TR.groups_to_labels(q, NESTED, threshold=0.85).tolist() == [1, 1, 2, 0, 0, 1, 0, 0]
    assert TR.groups_to_labels(q, NESTED, threshold=(0.85, 0.05)).tolist() == [2, 2, 2, 2, 0, 1, 2, 2]
    bits = np.array([[[True, True], [True, False]], [[False, True], [False, False]]])
    assert TR.groups_to_labels(bits, NESTED).tolist() == [[2, 1], [2, 0]]
    # decoding undoes labels_to_groups for nested groups
    label = np.random.RandomState(0).randint(0, 3, size=(4, 5, 6))
    planes = np.moveaxis(TR.labels_to_groups(label, NESTED), 0, -1)
    assert np.array_equal(TR.groups_to_labels(planes.astype(bool), NESTED), label)
    assert np.array_equal(TR.groups_to_labels(planes.astype(np.float32), NESTED), label)
    for bad in (dict(group_labels=(1,)), dict(group_labels=(1, 256)), dict(threshold=(0.5, 0.5, 0.5)), dict(threshold=nan)):
        with pytest.raises(ValueError):
            TR.groups_to_labels(q, NESTED, **bad)
    with pytest.raises(ValueError):
        TR.groups_to_labels(np.zeros((4, 3), dtype=np.float32), NESTED)


# --------------------------------------------------------------------------- host losses
def draw_groups(k, t, seed):
    """k distinct non-empty groups of label values below t, from a fixed seed."""
    rng = np.random.RandomState(seed)
    seen, out = set(), []
    while len(out) < k:
        g = tuple(sorted(rng.choice(t, size=rng.randint(1, 4), replace=False).tolist()))
        if g not in seen:
            seen.add(g)
            out.append(g)
    return tuple(out)


def make(kind, groups, gamma=2, **kw):
    cls = getattr(L, kind)
    if kind in ("GroupHybirdLoss", "GroupFocalLoss"):
        kw["gamma"] = gamma
    if kind == "GroupFocalLoss":
        for name in ("alpha", "beta", "smooth"):
            kw.pop(name, None)
    return cls(groups, **kw)


def formula(kind, z, y, groups, num_labels=None, ignore_label=None, gamma=2, weight_v=None, alpha=0.5, beta=0.5,
            smooth=1e-7):
    """The definitions, written out in float64 channel by channel."""
    z = z.double()
    n, k = z.shape[:2]
    zf = z.reshape(n, k, -1)
    yf = y.long().reshape(n, -1)
    counted = torch.ones_like(yf, dtype=torch.bool) if ignore_label is None else yf != ignore_label
    m = max(int(counted.sum()), 1)
    w = torch.ones(k, dtype=torch.float64) if weight_v is None else torch.tensor(weight_v, dtype=torch.float64)
    w = w / w.abs().sum().clamp_min(1e-12)
    total = 0.0
    for c, group in enumerate(groups):
        g = torch.zeros_like(yf, dtype=torch.bool)
        for t in group:
            g |= yf == t
        zc = zf[:, c][counted]
        gc = g[counted].double()
        p = torch.sigmoid(zc)
        tp, sp, sg = (p * gc).sum(), p.sum(), gc.sum()
        dice = (tp + smooth) / (tp + alpha * (sg - tp) + beta * (sp - tp) + smooth)
        logp, log1mp = -F.softplus(-zc), -F.softplus(zc)
        focal = (-(1 - p) ** gamma * gc * logp - p ** gamma * (1 - gc) * log1mp).sum() / m
        total = total + w[c] * {"GroupHybirdLoss": 1 - dice + focal, "GroupDiceLoss": 1 - dice, "GroupFocalLoss": focal,
                                "GroupDice": dice}[kind]
    return total


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k", [1, 3, 8])
def test_host_losses_equal_the_formula(kind, k):
    torch.manual_seed(10 * k)
    groups = draw_groups(k, 6, seed=k)
    z = torch.randn(2, k, 3, 4, 5, dtype=torch.float64) * 3
    y = torch.randint(0, 6, (2, 3, 4, 5))
    kw = dict(gamma=1.5, weight_v=[0.5 + c for c in range(k)], alpha=0.3, beta=0.7, smooth=1e-5)
    got = make(kind, groups, num_labels=6, **kw)(z, y)
    assert got.dim() == 0 and got.dtype == torch.float64
    want = formula(kind, z, y, groups, **kw)
    assert abs(float(got) - float(want)) <= 1e-12 * max(1.0, abs(float(want)))
    # defaults, uint8 labels, float32 logits
    got32 = make(kind, groups)(z.float(), y.to(torch.uint8))
    assert got32.dtype == torch.float32
    assert abs(float(got32) - float(formula(kind, z.float(), y, groups))) <= 1e-5


def test_focal_with_gamma_zero_is_binary_cross_entropy():
    torch.manual_seed(2)
    groups = ((1, 2), (2,), (3, 0))
    z = torch.randn(2, 3, 3, 4, 5, dtype=torch.float64) * 4
    y = torch.randint(0, 4, (2, 3, 4, 5))
    multi_hot = torch.from_numpy(TR.labels_to_groups(y.numpy(), groups)).movedim(0, 1).double()
    want = torch.stack([F.binary_cross_entropy_with_logits(z[:, c], multi_hot[:, c], reduction='mean')
                        for c in range(3)]).mean()
    got = L.GroupFocalLoss(groups, gamma=0)(z, y)
    assert abs(float(got) - float(want)) <= 1e-13


@pytest.mark.parametrize("kind", KINDS)
def test_host_losses_gradcheck(kind):
    torch.manual_seed(4)
    groups = ((1, 2), (2,), (0, 3))
    z = (torch.randn(2, 3, 2, 3, 2, dtype=torch.float64) * 2).requires_grad_(True)
    y = torch.randint(0, 4, (2, 2, 3, 2))
    y[0, 0, 0, 0] = 255
    crit = make(kind, groups, gamma=1.5, ignore_label=255, weight_v=[1.0, 2.0, 0.5], alpha=0.3, beta=0.7, smooth=1e-3)
    assert torch.autograd.gradcheck(lambda t: crit(t, y), (z,), eps=1e-6, atol=1e-7)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("ignore,dtype", [(255, torch.uint8), (-1, torch.int64)])
def test_ignore_label_equals_the_compacted_loss(kind, ignore, dtype):
    torch.manual_seed(6)
    groups = ((1, 2), (2,))
    z = torch.randn(1, 2, 4, 5, 6, dtype=torch.float64, requires_grad=True)
    y = torch.randint(0, 3, (1, 4, 5, 6))
    drop = torch.rand(1, 4, 5, 6) < 0.3
    yi = torch.where(drop, torch.full_like(y, ignore), y).to(dtype)
    got = make(kind, groups, ignore_label=ignore)(z, yi)
    keep = ~drop.reshape(-1)
    zc = z.reshape(1, 2, -1)[:, :, keep]
    want = make(kind, groups)(zc, y.reshape(1, -1)[:, keep])
    assert abs(float(got.detach()) - float(want.detach())) <= 1e-13
    assert abs(float(got.detach()) - float(formula(kind, z.detach(), yi, groups, ignore_label=ignore))) <= 1e-13
    got.backward()
    assert bool((z.grad[:, :, drop[0]] == 0).all()) and bool((z.grad[:, :, ~drop[0]] != 0).any())


@pytest.mark.parametrize("kind", KINDS)
def test_an_all_ignored_batch_is_finite_with_a_zero_gradient(kind):
    z = torch.randn(2, 2, 3, 3, 3, requires_grad=True)
    y = torch.full((2, 3, 3, 3), 255, dtype=torch.uint8)
    v = make(kind, NESTED, ignore_label=255)(z, y)
    v.backward()
    assert bool(torch.isfinite(v)) and bool((z.grad == 0).all())
    assert float(v.detach()) == {"GroupHybirdLoss": 0.0, "GroupDiceLoss": 0.0, "GroupFocalLoss": 0.0, "GroupDice": 1.0}[kind]


def test_host_argument_errors():
    z = torch.randn(1, 2, 3, 3, 3)
    y = torch.randint(0, 3, (1, 3, 3, 3))
    with pytest.raises(ValueError):
        L.GroupHybirdLoss(((1, 2), (2,), (1,)))(z, y)                    # three groups, two channels
    with pytest.raises(ValueError):
        L.GroupHybirdLoss(NESTED, weight_v=[1.0])
    with pytest.raises(N.Ru3dError):
        L.GroupHybirdLoss(NESTED)(z, y[:, :2])
    with pytest.raises(RuntimeError, match="Class values must be smaller than num_classes."):
        L.GroupHybirdLoss(NESTED)(z, torch.full_like(y, 3))
    assert isinstance(L.GroupHybirdLoss(NESTED), L._FusedLoss) and isinstance(L.GroupDice(NESTED), L._FusedLoss)


# --------------------------------------------------------------------------- evaluate_groups_case
def test_evaluate_groups_case_on_numpy_volumes():
    rng = np.random.RandomState(5)
    label = rng.randint(0, 4, size=(9, 8, 7)).astype(np.uint8)
    pred = np.where(rng.rand(9, 8, 7) < 0.7, label, rng.randint(0, 4, size=(9, 8, 7))).astype(np.uint8)
    groups = ((1, 2), (2,), (3, 1), (5,), (4, 6))                       # 5, and 4 with 6, are absent from both maps
    got = T.evaluate_groups_case({'label': label, 'pred': pred}, groups)
    assert len(got) == 5 and all(isinstance(v, float) for v in got)
    for k, g in enumerate(groups):
        a, b = np.isin(label, g), np.isin(pred, g)
        tp = float((a & b).sum())
        want = (tp + 1e-7) / (tp + 0.5 * (a & ~b).sum() + 0.5 * (~a & b).sum() + 1e-7)
        assert got[k] == pytest.approx(want, rel=1e-12), k
    assert got[3] == 1.0 and got[4] == 1.0
    assert 0.5 < got[0] < 1.0
    # a group the prediction misses entirely, and another smooth
    none = T.evaluate_groups_case({'label': label, 'pred': np.zeros_like(label)}, ((1, 2),), smooth=1e-3)
    assert none[0] == pytest.approx(1e-3 / (0.5 * np.isin(label, (1, 2)).sum() + 1e-3), rel=1e-12)
    assert T.evaluate_groups_case({'label': label, 'pred': label}, groups) == [1.0] * 5
    with pytest.raises(ValueError):
        T.evaluate_groups_case({'label': label, 'pred': pred}, ((1, 1),))


# --------------------------------------------------------------------------- C entry points
def test_names_in_header_bindings_library_and_makefile():
    header = open(os.path.join(ROOT, "include", "ru3d.h")).read()
    raw = ctypes.CDLL(N.LIB_PATH)
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in N.SIGNATURES and hasattr(N.lib, name) and hasattr(raw, name), name
    pkg = os.path.dirname(os.path.abspath(N.__file__))
    makefile = open(os.path.join(pkg, "csrc", "Makefile")).read()
    assert makefile.count("groups.hip") == 1                                                  # once: no 16-bit twin
    assert re.search(r"^SRCS\s*:=.*\bgroups\.hip\b", makefile, re.M)
    # the state begins like the softmax losses': the bad-label count sits at the shared offset
    assert N.lib.ru3d_group_loss_state_bytes() >= N.lib.ru3d_loss_state_bad_labels_offset() + 4
    for name in ("group_table", "GroupDice", "GroupDiceLoss", "GroupFocalLoss", "GroupHybirdLoss"):
        assert hasattr(L, name), name
    for name in ("labels_to_groups", "groups_to_labels", "default_group_labels"):
        assert hasattr(TR, name), name
    for name in ("evaluate_groups_case", "evaluate_groups", "batch_evaluate_groups"):
        assert hasattr(T, name), name


def test_workspace_query_has_a_slot_for_the_counted_voxels():
    lib = N.lib
    for n, v in ((1, 1), (2, 5 * 6 * 7), (2, 128 ** 3)):
        assert lib.ru3d_group_loss_workspace_bytes(n, v, 3) >= lib.ru3d_loss_workspace_bytes(n, v, 3) // 33 * 34


def test_c_argument_checks_answer_before_any_launch():
    lib = N.lib
    fake, other = ctypes.c_void_p(4096), ctypes.c_void_p(8192)                  # never dereferenced on these paths
    table = L.group_table(NESTED)

    def failed(rc, word):
        return rc < 0 and word in lib.ru3d_last_error()

    ws = lib.ru3d_group_loss_workspace_bytes(2, 512, 2)
    assert ws > 0

    def fwd(logits=fake, labels=fake, dtype=N.LABEL_I64, n=2, v=512, k=2, tab=table, t=3, has_ignore=0, ignore=0,
            kind=N.LOSS_HYBIRD, state=fake, out=fake, w=other, nbytes=ws):
        return lib.ru3d_group_loss_fwd(logits, 2 * 512, 512, 1, labels, dtype, n, v, k, tab, t, has_ignore, ignore, kind,
                                       2.0, None, 0.5, 0.5, 1e-7, state, out, w, nbytes, None)

    for name in ("logits", "labels", "state", "out", "w", "tab"):
        assert failed(fwd(**{name: None}), b"null"), name
    assert failed(fwd(k=0), b"groups unsupported")
    assert failed(fwd(k=9), b"groups unsupported")
    assert failed(fwd(t=33, tab=bytes(33)), b"label values unsupported")
    assert failed(fwd(t=0), b"label values unsupported")
    assert failed(fwd(nbytes=ws - 1), b"workspace")
    assert failed(fwd(nbytes=0), b"workspace")
    assert failed(fwd(n=0), b"empty")
    assert failed(fwd(v=0), b"empty")
    assert failed(fwd(kind=4), b"bad kind")
    assert failed(fwd(dtype=7), b"label dtype")
    assert failed(fwd(has_ignore=1, ignore=2), b"ignore label")
    assert failed(fwd(k=1), b"member of a group above")                          # the table has bit 1 set

    def bwd(logits=fake, labels=fake, dtype=N.LABEL_U8, n=2, v=512, k=2, tab=table, t=3, has_ignore=0, ignore=0,
            state=fake, dz=fake, dz_dtype=N.F32):
        return lib.ru3d_group_loss_bwd(logits, 2 * 512, 512, 1, labels, dtype, n, v, k, tab, t, has_ignore, ignore, 2.0,
                                       state, None, dz, dz_dtype, None)

    for name in ("logits", "labels", "state", "dz", "tab"):
        assert failed(bwd(**{name: None}), b"null"), name
    assert failed(bwd(k=0), b"groups unsupported")
    assert failed(bwd(k=9), b"groups unsupported")
    assert failed(bwd(t=33, tab=bytes(33)), b"label values unsupported")
    assert failed(bwd(n=0), b"empty")
    assert failed(bwd(dtype=-1), b"label dtype")
    assert failed(bwd(dz_dtype=N.F16), b"dlogits dtype")
    assert failed(bwd(has_ignore=1, ignore=0), b"ignore label")

    def tensor(c=2, n=1, ptr=4096):
        return N.Tensor(ptr, n, 8, 8, 8, c, c, 0, 0)

    def acc(t=None, dtype=N.F32, sample=0, flip=0, tables=(None, None, None), a=fake, cnt=other, vol=(13, 11, 17),
            origin=(0, 0, 0)):
        t = tensor() if t is None else t
        return lib.ru3d_predict_accumulate_groups(ctypes.byref(t), dtype, sample, flip, tables[0], tables[1], tables[2],
                                                  a, cnt, vol[0], vol[1], vol[2], origin[0], origin[1], origin[2], None)

    assert failed(acc(t=tensor(ptr=None)), b"bad argument")
    assert failed(acc(a=None), b"bad argument")
    assert failed(acc(cnt=None), b"bad argument")
    assert failed(acc(t=tensor(c=9)), b"9 groups")
    assert failed(acc(dtype=N.F16), b"dtype")
    assert failed(acc(sample=1), b"sample")
    assert failed(acc(flip=8), b"mirror mask")
    assert failed(acc(tables=(fake, None, fake)), b"weight tables")
    for origin in ((6, 0, 0), (0, 4, 0), (0, 0, 10), (-1, 0, 0)):
        assert failed(acc(origin=origin), b"outside"), origin
    assert failed(acc(vol=(7, 11, 17)), b"outside")

    labels, thr = (ctypes.c_int32 * 2)(1, 2), (ctypes.c_float * 2)(0.5, 0.5)

    def merge(a=fake, cnt=other, vol=(13, 11, 17), k=2, lab=labels, th=thr, crop=(0, 0, 0), size=(13, 11, 17), out=fake):
        return lib.ru3d_predict_merge_groups(a, cnt, vol[0], vol[1], vol[2], k, lab, th, crop[0], crop[1], crop[2],
                                             size[0], size[1], size[2], out, None)

    for name in ("a", "cnt", "lab", "th", "out"):
        assert failed(merge(**{name: None}), b"bad argument"), name
    assert failed(merge(k=0), b"0 groups")
    assert failed(merge(k=9), b"9 groups")
    assert failed(merge(crop=(1, 0, 0)), b"outside")
    assert failed(merge(size=(13, 11, 18)), b"outside")
    assert failed(merge(size=(0, 11, 17)), b"outside")
    assert failed(merge(lab=(ctypes.c_int32 * 2)(1, 256)), b"label 256")
    assert failed(merge(th=(ctypes.c_float * 2)(0.5, float("nan"))), b"NaN")
