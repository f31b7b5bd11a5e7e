"""CPU-only checks of the boundary-loss feature: the numpy twin of loss.signed_distance_map (the definition the HIP kernels
are held to) against a brute force over all voxel pairs, the degenerate rules (a class absent from a sample or filling
it), the patch faces, BoundaryLoss on host tensors against the formula written out here and under gradcheck, argument
handling in Python and in the C entry points (which answer before any launch), and the names in the header, the
bindings, the library and the Makefile."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _native as N
import loss as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["ru3d_boundary_workspace_bytes", "ru3d_boundary_state_bytes", "ru3d_signed_distance", "ru3d_boundary_fwd",
                "ru3d_boundary_bwd"]


# ------------------------------------------------------------------------------------------------ brute force
def brute_signed_squares(g):
    """int64 array like g: +min |v - u|^2 over u in G for v outside, -min over u outside G for v inside; every pair of
    voxels is visited.  Zeros when G is empty or everything."""
    out = np.zeros(g.shape, dtype=np.int64)
    if not g.any() or g.all():
        return out
    p = np.indices(g.shape).reshape(3, -1).T.astype(np.int64)
    d2 = ((p[:, None, :] - p[None, :, :]) ** 2).sum(-1)
    flat = g.reshape(-1)
    big = np.iinfo(np.int64).max
    to_fg = np.where(flat[None, :], d2, big).min(axis=1)
    to_bg = np.where(~flat[None, :], d2, big).min(axis=1)
    return np.where(flat, -to_bg, to_fg).reshape(g.shape)


def brute_maps(labels, classes):
    lab = labels.numpy()
    return np.stack([np.stack([brute_signed_squares(lab[n] == q) for q in classes]) for n in range(lab.shape[0])])


def phi_of(d2):
    """float32(sqrt(float64(d2))) with the sign rule, in numpy."""
    root = np.sqrt(np.abs(d2).astype(np.float64)).astype(np.float32)
    return np.where(d2 < 0, -(root - np.float32(1)), root).astype(np.float32)


def twin_cases():
    gen = torch.Generator().manual_seed(3)
    blobs = torch.randint(0, 3, (2, 6, 5, 7), generator=gen)
    line = torch.zeros((1, 1, 1, 70), dtype=torch.int64)
    line[0, 0, 0, 5:9] = 1
    line[0, 0, 0, 64:66] = 2
    line[0, 0, 0, 69] = 1
    single = torch.ones((1, 1, 1, 1), dtype=torch.int64)
    return [("blobs", blobs, (1, 2)), ("blobs reversed", blobs, (2, 1)), ("blobs class 0", blobs, (0,)),
            ("line", line, (1, 2)), ("single voxel", single, (1, 2))]


@pytest.mark.parametrize("name,labels,classes", twin_cases(), ids=[c[0] for c in twin_cases()])
def test_twin_equals_the_brute_force(name, labels, classes):
    want = brute_maps(labels, classes)
    sq = L.signed_distance_map(labels, 3, classes=classes, squared=True)
    assert sq.dtype == torch.int32 and tuple(sq.shape) == (labels.shape[0], len(classes)) + tuple(labels.shape[1:])
    assert np.array_equal(sq.numpy().astype(np.int64), want), name
    phi = L.signed_distance_map(labels, 3, classes=classes)
    assert phi.dtype == torch.float32 and phi.shape == sq.shape
    assert np.array_equal(phi.numpy(), phi_of(want)), name
    if name == "single voxel":
        assert not sq.any() and not phi.any()
    else:
        assert bool((sq != 0).all())                     # two kinds present: no voxel is at distance 0 from the other
        # foreground voxels on the boundary: d2 = 1 inside, phi = 0
        assert bool((phi[sq == -1] == 0).all()) and bool((phi[sq == 1] == 1).all())


def test_default_classes_and_label_dtypes():
    labels = twin_cases()[0][1]
    want = L.signed_distance_map(labels, 3, classes=(1, 2), squared=True)
    assert torch.equal(L.signed_distance_map(labels, 3, squared=True), want)
    assert torch.equal(L.signed_distance_map(labels.to(torch.uint8), 3, squared=True), want)
    assert torch.equal(L.signed_distance_map(labels.to(torch.int32), 3, squared=True), want)


def test_absent_and_filling_classes_give_zeros_for_that_sample_only():
    labels = twin_cases()[0][1].clone()
    labels[0][labels[0] == 2] = 0                        # class 2 absent from sample 0, present in sample 1
    sq = L.signed_distance_map(labels, 3, classes=(1, 2), squared=True)
    phi = L.signed_distance_map(labels, 3, classes=(1, 2))
    assert not sq[0, 1].any() and not phi[0, 1].any()
    assert sq[1, 1].all() and sq[0, 0].all()
    assert np.array_equal(sq.numpy().astype(np.int64), brute_maps(labels, (1, 2)))
    labels[1] = 1                                        # class 1 fills sample 1 (so class 2 is absent there as well)
    sq = L.signed_distance_map(labels, 3, classes=(1, 2), squared=True)
    assert not sq[1].any() and sq[0, 0].all()
    assert not L.signed_distance_map(labels, 3, classes=(1, 2))[1].any()
    # a label outside [0, C) matches no class: background of every selected class
    odd = twin_cases()[0][1].clone()
    odd[0, 2, 2, 3] = 7
    as_background = odd.clone()
    as_background[0, 2, 2, 3] = 0
    assert torch.equal(L.signed_distance_map(odd, 3, squared=True), L.signed_distance_map(as_background, 3, squared=True))


def test_patch_faces_are_not_a_boundary():
    labels = torch.zeros((1, 6, 6, 6), dtype=torch.int64)
    labels[0, :3, :, :] = 1                              # a slab that touches five faces; its only boundary is a = 2 | 3
    sq = L.signed_distance_map(labels, 2, squared=True)[0, 0]
    for a in range(6):
        want = -(3 - a) ** 2 if a < 3 else (a - 2) ** 2
        assert bool((sq[a] == want).all()), a
    phi = L.signed_distance_map(labels, 2)[0, 0]
    assert phi[0].unique().tolist() == [-2.0] and phi[2].unique().tolist() == [0.0] and phi[5].unique().tolist() == [3.0]


# ------------------------------------------------------------------------------------------------ the loss on the host
def formula(logits, labels, classes, weight_v):
    """loss = sum_q w_q / (N V) sum_n sum_v P_q phi_q written out in numpy float64."""
    c = logits.shape[1]
    z = logits.double().numpy()
    e = np.exp(z - z.max(axis=1, keepdims=True))
    p = e / e.sum(axis=1, keepdims=True)
    cls = list(range(1, c)) if classes is None else list(classes)
    w = np.array([1.0 if weight_v is None else weight_v[q] for q in cls], dtype=np.float64)
    w = w / np.abs(w).sum()
    phi = phi_of(brute_maps(labels, cls)).astype(np.float64)
    total = 0.0
    for k, q in enumerate(cls):
        total += w[k] * (p[:, q] * phi[:, k]).sum() / (logits.shape[0] * np.prod(logits.shape[2:]))
    return total


@pytest.mark.parametrize("classes,weight_v", [(None, None), ((2,), None), ((0, 2), [0.2, 0.5, 3.0]), ((2, 1), [1.0, 2.0, 0.5])])
def test_boundary_loss_is_the_formula(classes, weight_v):
    gen = torch.Generator().manual_seed(23)
    logits = torch.randn((2, 3, 6, 5, 7), dtype=torch.float64, generator=gen) * 2
    labels = torch.randint(0, 3, (2, 6, 5, 7), generator=gen)
    got = L.BoundaryLoss(weight_v=weight_v, classes=classes)(logits, labels)
    assert got.dim() == 0 and got.dtype == torch.float64
    want = formula(logits, labels, classes, weight_v)
    assert abs(float(got) - want) <= 1e-12 * max(1.0, abs(want))


def test_boundary_loss_gradcheck():
    gen = torch.Generator().manual_seed(29)
    logits = torch.randn((1, 3, 4, 3, 5), dtype=torch.float64, generator=gen).requires_grad_(True)
    labels = torch.randint(0, 3, (1, 4, 3, 5), generator=gen)
    crit = L.BoundaryLoss(weight_v=[0.5, 1.0, 2.0])
    assert torch.autograd.gradcheck(lambda z: crit(z, labels), (logits,))
    crit(logits, labels).backward()
    # softmax: the gradient over the classes of a voxel sums to zero
    assert float(logits.grad.sum(1).abs().max()) <= 1e-15 and float(logits.grad.abs().max()) > 0


def test_an_absent_class_gives_no_loss_and_no_gradient():
    gen = torch.Generator().manual_seed(31)
    logits = torch.randn((1, 3, 4, 3, 5), dtype=torch.float64, generator=gen).requires_grad_(True)
    labels = torch.randint(0, 2, (1, 4, 3, 5), generator=gen)            # class 2 absent
    v = L.BoundaryLoss(classes=(2,))(logits, labels)
    v.backward()
    assert float(v.detach()) == 0.0 and float(logits.grad.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ arguments, names
def test_argument_errors():
    y5 = torch.zeros(1, 4, 4, 4, dtype=torch.int64)
    with pytest.raises(N.Ru3dError, match="no CPU fallback"):
        L.HybirdBoundaryLoss()(torch.zeros(1, 2, 4, 4, 4), y5)
    with pytest.raises(N.Ru3dError, match="C == 1"):
        L.BoundaryLoss()(torch.zeros(1, 1, 4, 4, 4), y5)
    with pytest.raises(N.Ru3dError, match="three spatial"):
        L.BoundaryLoss()(torch.zeros(1, 2, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64))
    for bad in ((1, 1), (3,), (-1,), ()):
        with pytest.raises(N.Ru3dError, match="classes"):
            L.BoundaryLoss(classes=bad)(torch.zeros(1, 3, 4, 4, 4), y5)
        with pytest.raises(N.Ru3dError, match="classes"):
            L.signed_distance_map(y5, 3, classes=bad)
    with pytest.raises(RuntimeError, match="weight_v has 2 entries for 3 classes"):
        L.BoundaryLoss(weight_v=[1.0, 2.0])(torch.zeros(1, 3, 4, 4, 4), y5)
    with pytest.raises(N.Ru3dError, match="integer labels"):
        L.signed_distance_map(torch.zeros(1, 4, 4, 4), 3)
    with pytest.raises(N.Ru3dError, match="integer labels"):
        L.signed_distance_map(torch.zeros(4, 4, 4, dtype=torch.int64), 3)
    with pytest.raises(N.Ru3dError, match="target shape"):
        L.BoundaryLoss()(torch.zeros(1, 2, 4, 4, 4), torch.zeros(1, 4, 4, 5, dtype=torch.int64))
    assert issubclass(L.BoundaryLoss, L._FusedLoss) and issubclass(L.HybirdBoundaryLoss, L._FusedLoss)


def test_boundary_weight_buffer_and_property():
    crit = L.HybirdBoundaryLoss()
    assert crit.boundary_weight == 0.01
    state = crit.state_dict()
    assert list(state) == ["boundary_weight_buffer"] and state["boundary_weight_buffer"].dtype == torch.float32
    assert state["boundary_weight_buffer"].tolist() == [float(np.float32(0.01))]
    crit.set_boundary_weight(0.25)
    assert crit.boundary_weight == 0.25 and crit.state_dict()["boundary_weight_buffer"].tolist() == [0.25]
    with pytest.raises(AttributeError):
        crit.boundary_weight = 0.5
    other = L.HybirdBoundaryLoss(boundary_weight=0.5)
    other.load_state_dict(crit.state_dict())
    assert other.boundary_weight == 0.25 and other.boundary_weight_buffer.tolist() == [0.25]


def test_names_in_header_bindings_library_and_makefile():
    header = open(os.path.join(ROOT, "include", "ru3d.h")).read()
    raw = ctypes.CDLL(N.LIB_PATH)
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in N.SIGNATURES and hasattr(N.lib, name) and hasattr(raw, name), name
    pkg = os.path.dirname(os.path.abspath(N.__file__))
    assert open(os.path.join(pkg, "csrc", "Makefile")).read().count("boundary.hip") == 1        # once: no 16-bit twin
    assert N.lib.ru3d_version() == 201
    assert N.BOUNDARY_MAX_AXIS == int(re.search(r"#define RU3D_BOUNDARY_MAX_AXIS (\d+)", header).group(1)) >= 512
    # 3 (L - 1)^2 of the largest legal extent is exact in float32 and far inside int32
    assert 3 * (N.BOUNDARY_MAX_AXIS - 1) ** 2 < 2 ** 24
    assert "unit spacing" in header and "sampling" in header
    assert N.lib.ru3d_boundary_state_bytes() >= N.lib.ru3d_loss_state_bad_labels_offset() + 4


def test_workspace_query():
    lib = N.lib
    lim = N.BOUNDARY_MAX_AXIS
    v = 128 ** 3
    # the documented layout: one int32 plane and one bit per voxel of every volume, and a little in front
    assert lib.ru3d_boundary_workspace_bytes(4, 128, 128, 128) >= 4 * v * 4 + 4 * v // 8
    assert lib.ru3d_boundary_workspace_bytes(1, 1, 1, 1) > 0
    assert lib.ru3d_boundary_workspace_bytes(1, lim, 4, 4) > 0 and lib.ru3d_boundary_workspace_bytes(1, 4, 4, lim) > 0
    for shape in ((lim + 1, 4, 4), (4, lim + 1, 4), (4, 4, lim + 1), (0, 4, 4), (4, -1, 4), (2048, 2048, 2048)):
        assert lib.ru3d_boundary_workspace_bytes(1, *shape) == 0, shape
    assert lib.ru3d_boundary_workspace_bytes(0, 4, 4, 4) == 0


def test_c_argument_checks_answer_before_any_launch():
    lib = N.lib
    fake, other = ctypes.c_void_p(4096), ctypes.c_void_p(8192)                  # never dereferenced on these paths
    lim = N.BOUNDARY_MAX_AXIS

    def classes(*cls):
        return ctypes.cast((ctypes.c_int * max(len(cls), 1))(*cls), ctypes.c_void_p)

    def failed(rc, word):
        return rc < 0 and word in lib.ru3d_last_error()

    ws = lib.ru3d_boundary_workspace_bytes(4, 8, 8, 8)
    ok = classes(1, 2)

    def sd(labels=fake, dtype=N.LABEL_U8, n=2, shape=(8, 8, 8), c=3, cls=ok, nsel=2, d2=fake, phi=fake, w=other,
           nbytes=ws):
        return lib.ru3d_signed_distance(labels, dtype, n, shape[0], shape[1], shape[2], c, cls, nsel, d2, phi, w, nbytes,
                                        None)

    assert failed(sd(labels=None), b"null")
    assert failed(sd(w=None), b"null")
    assert failed(sd(d2=None, phi=None), b"null")
    assert failed(sd(cls=None), b"null")
    assert failed(sd(dtype=7), b"label dtype")
    assert failed(sd(nsel=0), b"class selection")
    assert failed(sd(nsel=4), b"class selection")
    assert failed(sd(cls=classes(1, 3)), b"class 3 out of range")
    assert failed(sd(cls=classes(-1, 2)), b"class -1 out of range")
    assert failed(sd(cls=classes(2, 2)), b"selected twice")
    assert failed(sd(c=1, cls=classes(0), nsel=1), b"classes (2 .. 8)")
    assert failed(sd(c=9), b"classes (2 .. 8)")
    assert failed(sd(n=0), b"empty")
    assert failed(sd(shape=(8, 0, 8)), b"empty")
    assert failed(sd(shape=(lim + 1, 8, 8)), b"limit of %d" % lim)
    assert failed(sd(shape=(8, lim + 1, 8)), b"limit of %d" % lim)
    assert failed(sd(shape=(8, 8, lim + 1)), b"limit of %d" % lim)
    assert failed(sd(shape=(2048, 2048, 2048)), b"2^31")
    assert failed(sd(nbytes=ws - 1), b"workspace")
    assert failed(sd(nbytes=0), b"workspace")

    def fwd(logits=fake, labels=fake, dtype=N.LABEL_I64, n=2, shape=(8, 8, 8), c=3, cls=ok, nsel=2, phi=fake, state=fake,
            out=fake, w=other, nbytes=ws):
        return lib.ru3d_boundary_fwd(logits, 3 * 512, 512, 1, labels, dtype, n, shape[0], shape[1], shape[2], c, cls, nsel,
                                     None, phi, state, out, w, nbytes, None)

    for name in ("logits", "labels", "phi", "state", "out", "w", "cls"):
        assert failed(fwd(**{name: None}), b"null"), name
    assert failed(fwd(dtype=-1), b"label dtype")
    assert failed(fwd(nsel=0), b"class selection")
    assert failed(fwd(cls=classes(0, 3)), b"class 3 out of range")
    assert failed(fwd(shape=(8, 8, lim + 1)), b"limit of %d" % lim)
    assert failed(fwd(nbytes=ws - 1), b"workspace")

    def bwd(logits=fake, n=2, shape=(8, 8, 8), c=3, cls=ok, nsel=2, phi=fake, state=fake, dz=fake):
        return lib.ru3d_boundary_bwd(logits, 3 * 512, 512, 1, n, shape[0], shape[1], shape[2], c, cls, nsel, phi, state,
                                     None, 1.0, 0, dz, None)

    for name in ("logits", "phi", "state", "dz", "cls"):
        assert failed(bwd(**{name: None}), b"null"), name
    assert failed(bwd(nsel=0), b"class selection")
    assert failed(bwd(cls=classes(3, 1)), b"class 3 out of range")
    assert failed(bwd(shape=(lim + 1, 8, 8)), b"limit of %d" % lim)
    assert failed(bwd(n=-1), b"empty")
