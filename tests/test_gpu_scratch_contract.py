"""The memory contracts of the losses, the post-processing and the data ops: every entry point outside the conv and norm
families that carves scratch out of _native.workspace() or allocates state, outputs and capacity buffers with
torch.empty, one case per wrapper call, on a real MI355X.  tests/test_gpu_conv_contract.py (section A) is the model; its
hostile stand-ins are restated here because these wrappers live in a dozen modules, some of which import torch inside
their functions: the stand-in replaces torch.empty / empty_like / empty_strided themselves for the length of one call.

Shapes (the smallest at which a layout has more than one row per region and a ragged tail):
  packed-mask and volume ops  (9, 10, 67) voxels: three 2048-voxel chunks, the last partial; Z straddles a 64-bit word
  losses                      logits (2, C, 8, 10, 68), labels (2, 8, 10, 68): six 2048-voxel partial rows, the last partly
                              filled; deep supervision adds the level (4, 5, 34)
  patch samplers              patch (5, 9, 70) out of a (12, 14, 80) case, two channels

Checks per case, in this order:
  1  reference     the clean run against the reference and the tolerance of the case's own test file (scipy, the numpy
                   twin, the float64 host twin)
  2  determinism   two clean runs: the same bits
  3  leftovers     0x00, 0xFF, 0x7F in every buffer of _native._WS and in everything the wrapper allocates: the same bits
                   as the clean run (so no NaN the clean run had not); for the losses the backward too, and the label
                   verdict does not move
  4  exact size    a private scratch of exactly each ask, NaN-filled, a 0xA5 guard behind it: the same bits, guard
                   untouched; every value the case's *_workspace_bytes / *_state_bytes queries return is covered by an ask
  5  short         each ask in turn 16 bytes short: Ru3dError, no launch after the ask and none ahead of the first ask (the
                   launch log of the whole call is empty; AHEAD names the three wrappers that launch an entry point
                   without scratch first), nothing the wrapper allocated changes after the ask (what it allocates later
                   keeps its fill), guards untouched
  6  edges         every PackedMask a case returns has its padding bits at z >= Z clear, in every run of 1 .. 4; every
                   allocation of the wrapper has a guard of its own behind it, checked after every run; where only a
                   counted prefix of a capacity buffer is valid the case returns that prefix and says so

The post-processing cases (morphometry, floods, keep-largest, the vessel graph, territories, geodesic growth) take their
host volumes from tests/contract_inputs.py; tests/test_host_contract_inputs.py holds those volumes, without a device, to
what each case is there to exercise (a second batch of rounds, a tie, an empty id, ..).

Two coverage tests at the end hold the case table against _native.SIGNATURES: every *_workspace_bytes / *_state_bytes
query is named by a case, and every entry point is called by the clean run of a case or listed, with the test file that
holds it, in HELD_ELSEWHERE.
Run with `-m gpu`."""
import contextlib
import functools
import math
import os

import numpy as np
import pytest
import scipy.ndimage as ndi
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no HIP device", allow_module_level=True)

import _native as N  # noqa: E402
import _ops as ops  # noqa: E402
import augment  # noqa: E402
import components  # noqa: E402
import degrade  # noqa: E402
import distance  # noqa: E402
import geodesic  # noqa: E402
import loss as L  # noqa: E402
import mesh  # noqa: E402
import morphology  # noqa: E402
import morphometry  # noqa: E402
import prepare  # noqa: E402
import skeleton  # noqa: E402
import territory  # noqa: E402
import trainer  # noqa: E402
import transform as T  # noqa: E402
import visualize as V  # noqa: E402
import contract_inputs as CI  # noqa: E402
import test_gpu_loss_contract as LC  # noqa: E402
import test_gpu_topk as TK  # noqa: E402
from test_host_skeleton_graph import same  # noqa: E402

DEV = torch.device("cuda:0")
LEFTOVERS = (0x00, 0xFF, 0x7F)
SHORT = 16
GUARD_MIN = 4 << 20         # behind a private scratch
GUARD_OUT = 64 << 10        # behind everything the wrapper allocates
VOL = (9, 10, 67)
LOSS_SPATIAL, LOSS_LEVEL1 = (8, 10, 68), (4, 5, 34)
CASE_SHAPE, PATCH, CHANNELS = (12, 14, 80), (5, 9, 70), 2
VALUE_TOL, GRAD_REL, GRAD_FLOOR = 2e-6, 2e-5, 1e-6      # tests/test_gpu_loss_kernels.py, _groups, _topk, _deepsup
EPS = 2.0 ** -23                                        # tests/test_gpu_augment_degrade.py

_EMPTY, _EMPTY_LIKE, _EMPTY_STRIDED = torch.empty, torch.empty_like, torch.empty_strided


# ------------------------------------------------------------------------------------------------ hostile stand-ins
class _Alloc:
    """stands in for torch.empty / empty_like / empty_strided around one call: every device tensor the wrapper allocates
    starts as `fill` bytes and (where it is contiguous) has a 0xA5 guard of its own behind it in the same allocation.
    shrink: {nbytes: n} - a uint8 allocation of exactly nbytes (a scratch the wrapper allocates itself) comes n short"""

    def __init__(self, fill=0xFF, shrink=None):
        self.fill, self.shrink, self.made, self.sizes = fill, shrink or {}, [], []

    def _new(self, shape, dtype, device):
        shape = tuple(int(s) for s in shape)
        nbytes = dtype.itemsize
        for extent in shape:
            nbytes *= extent
        if dtype == torch.uint8 and len(shape) == 1:
            self.sizes.append(nbytes)
            if nbytes in self.shrink:
                nbytes -= self.shrink[nbytes]
                shape = (nbytes,)
        buf = _EMPTY(nbytes + GUARD_OUT, dtype=torch.uint8, device=device)
        buf[:nbytes].fill_(self.fill)
        buf[nbytes:].fill_(0xA5)
        self.made.append((buf, nbytes))
        return buf[:nbytes].view(dtype).view(shape)

    def _filled(self, t):
        if t.is_cuda and t.numel():
            one = torch.full((t.element_size(),), self.fill, dtype=torch.uint8, device=t.device).view(t.dtype)
            t.copy_(one[0].expand(t.shape))
        return t

    @staticmethod
    def _on_device(device):
        return device is not None and torch.device(device).type == "cuda"

    def empty(self, *size, dtype=None, device=None, **kw):
        if len(size) == 1 and not isinstance(size[0], int):
            size = tuple(size[0])
        if kw or not self._on_device(device):
            return self._filled(_EMPTY(*size, dtype=dtype, device=device, **kw))
        return self._new(size, dtype or torch.get_default_dtype(), device)

    def empty_like(self, t, dtype=None, **kw):
        if kw or not t.is_cuda or not t.is_contiguous():
            return self._filled(_EMPTY_LIKE(t, dtype=dtype, **kw))
        return self._new(t.shape, dtype or t.dtype, t.device)

    def empty_strided(self, *a, **kw):
        return self._filled(_EMPTY_STRIDED(*a, **kw))

    def guards_intact(self):
        return all(bool((buf[size:] == 0xA5).all()) for buf, size in self.made)

    def snapshot(self):
        return [buf.clone() for buf, _ in self.made]

    def unchanged_since(self, snap):
        """the allocations of the snapshot hold what they held, the later ones their fill"""
        for i, (buf, size) in enumerate(self.made):
            if i < len(snap):
                if not torch.equal(buf, snap[i]):
                    return False
            elif not bool((buf[:size] == self.fill).all()):
                return False
        return True


class _Scratch:
    """stands in for N.workspace around one call: a private buffer per ask, of the asked size (ask number `only`: less
    `short` bytes), filled with NaN, with a guard of 0xA5 behind it in the same allocation (at least as large, never under
    4 MiB).  At the short ask the launch log so far is kept in `before` and starts anew, and `alloc` is photographed: what
    follows must launch nothing and write nothing"""

    def __init__(self, short=0, only=None, alloc=None):
        self.short, self.only, self.alloc, self.snap, self.before = short, only, alloc, None, None
        self.queries, self.bufs = [], []

    def __call__(self, nbytes, device, slot=0):
        nbytes = int(nbytes)
        short = self.short if self.only is None or self.only == len(self.queries) else 0
        size = max(nbytes - short, 0)
        buf = _EMPTY(size + max(nbytes, GUARD_MIN), dtype=torch.uint8, device=device)
        buf[:size].fill_(0xFF)
        buf[size:].fill_(0xA5)
        self.queries.append(nbytes)
        self.bufs.append((buf, size))
        if short:
            torch.cuda.synchronize()
            ahead = N.lib.ru3d_launch_log_end().decode("utf-8", "replace")
            self.before = ahead.split(";") if ahead else []
            N.lib.ru3d_launch_log_begin()
            if self.alloc is not None:
                self.snap = self.alloc.snapshot()
        return buf[:size]

    def guard_intact(self):
        return all(bool((buf[size:] == 0xA5).all()) for buf, size in self.bufs)


@contextlib.contextmanager
def _swapped(scratch=None, alloc=None):
    saved = N.workspace, torch.empty, torch.empty_like, torch.empty_strided
    try:
        if scratch is not None:
            N.workspace = scratch
        if alloc is not None:
            torch.empty, torch.empty_like, torch.empty_strided = alloc.empty, alloc.empty_like, alloc.empty_strided
        yield
    finally:
        N.workspace, torch.empty, torch.empty_like, torch.empty_strided = saved


@contextlib.contextmanager
def _spied(names):
    """the named queries of N.lib, recorded: {name: [returned values]}"""
    seen, saved = {n: [] for n in names}, {}
    for n in names:
        saved[n] = fn = getattr(N.lib, n)

        def spy(*a, _fn=fn, _n=n):
            r = _fn(*a)
            seen[_n].append(int(r))
            return r
        setattr(N.lib, n, spy)
    try:
        yield seen
    finally:
        for n, fn in saved.items():
            setattr(N.lib, n, fn)


def _padding_clear(mask, what):
    Z = mask.shape3[2]
    assert tuple(mask.bits.shape) == mask.shape3[:2] + ((Z + 63) // 64,) and mask.bits.dtype == torch.int64, what
    if Z & 63:
        tail = mask.bits[..., -1] >> (Z & 63)           # arithmetic shift: a set sign bit stays visible
        assert int(tail.ne(0).sum().item()) == 0, "%s: padding bits at z >= %d are set" % (what, Z)


def _flat(out, what):
    """the outputs of a call as {name: tensor}: a PackedMask gives its words (padding checked here, in every run), numbers
    and numpy arrays become tensors"""
    flat = {}
    for k, v in out.items():
        if isinstance(v, morphology.PackedMask):
            _padding_clear(v, "%s: %s" % (what, k))
            v = v.bits
        elif isinstance(v, np.ndarray):
            v = torch.from_numpy(np.ascontiguousarray(v))
        elif not torch.is_tensor(v):
            v = torch.tensor(v, dtype=torch.float64 if any(isinstance(e, float) for e in np.atleast_1d(v).tolist())
                             else torch.int64)
        flat[k] = v.detach().clone()
    return flat


def _run(call, what, scratch=None, alloc=None):
    """the one call inside the launch log -> (launch names, {name: tensor} or {}, Ru3dError message or None).  The
    backward of a loss runs on this thread too, so that its launches are logged and its scratch is this call's"""
    err, out = None, {}
    with torch.autograd.set_multithreading_enabled(False), _swapped(scratch, alloc):
        with ops.launch_log() as log:
            try:
                out = call()
                torch.cuda.synchronize()
            except N.Ru3dError as e:
                err = str(e)
    torch.cuda.synchronize()
    if alloc is not None:
        assert alloc.guards_intact(), "%s wrote behind a tensor it allocated" % what
    return log.names, (_flat(out, what) if err is None else {}), err


def _bits(t):
    if t.is_floating_point():
        return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])
    return t


def _same(a, b, what):
    assert a.keys() == b.keys(), what
    for k in a:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, (what, k, a[k].shape, b[k].shape)
        if not torch.equal(_bits(a[k]), _bits(b[k])):
            raise AssertionError("%s: %s differs in %d of %d elements" % (
                what, k, int((_bits(a[k]) != _bits(b[k])).sum()), a[k].numel()))


# ------------------------------------------------------------------------------------------------ the case table
# name -> (builder, the *_workspace_bytes / *_state_bytes queries the wrapper call goes through, kind)
CASES = {}


def case(name, queries=(), kind="op"):
    def deco(fn):
        CASES[name] = (functools.lru_cache(maxsize=None)(fn), tuple(queries), kind)
        return fn
    return deco


def _built(name):
    """(call, reference): call() makes the one wrapper call on operands that were uploaded once and returns its outputs
    by name; reference(outputs) holds the clean run to the reference of the wrapper's own test file"""
    return CASES[name][0]()


def _up(a):
    return torch.from_numpy(np.array(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def _volumes():
    """read-only host volumes of VOL: a speckle mask, sparse features, a solid with a tunnel, two label volumes"""
    rng = np.random.RandomState(67)
    mask = rng.rand(*VOL) < 0.45
    mask[0, 0, 0] = mask[-1, -1, -1] = True
    feat = rng.rand(*VOL) < 0.02
    feat[2, 3, 65] = True
    x, y, z = np.ogrid[:VOL[0], :VOL[1], :VOL[2]]
    solid = ((x - 4) ** 2 / 14.0 + (y - 4.5) ** 2 / 18.0 + (z - 33) ** 2 / 1000.0 < 1) & ~((abs(x - 4) < 1) & (abs(y - 5) < 2))
    solid |= (x == 7) & (y > 2) & (z > 50)
    pred = rng.randint(0, 5, VOL).astype(np.uint8)
    label = rng.randint(0, 5, VOL).astype(np.uint8)
    for a in (mask, feat, solid, pred, label):
        a.setflags(write=False)
    return dict(mask=mask, feat=feat, solid=solid, pred=pred, label=label)


def _pack(a):
    return morphology.pack(_up(a.astype(np.uint8)))


def _bools(packed_words, shape=VOL):
    """host bool volume of the words of a PackedMask [X, Y, W]"""
    w = packed_words.cpu().numpy().view(np.uint64)
    z = np.arange(shape[2])
    return ((w[..., z // 64] >> (z % 64).astype(np.uint64)) & np.uint64(1)).astype(bool)


def _edt_brute(features):
    """the contract of distance.edt_squared at unit spacing, A + (B + C) over integers: exact in float64"""
    return _edt_brute_of(features.tobytes(), features.shape)


@functools.lru_cache(maxsize=None)
def _edt_brute_of(data, shape):
    features = np.frombuffer(data, dtype=bool).reshape(shape)
    f = np.argwhere(features).astype(np.int64)
    p = np.indices(features.shape).reshape(3, -1).T.astype(np.int64)
    d = np.concatenate([((p[i:i + 256, None, :] - f[None, :, :]) ** 2).sum(-1).min(1) for i in range(0, len(p), 256)])
    return d.reshape(features.shape).astype(np.float64)


# ---- components.py (reference: scipy, tests/test_gpu_components.py, equality)
@case("components.label", ["ru3d_components_workspace_bytes"])
def _c_label():
    m, host = _up(_volumes()["mask"].astype(np.uint8)), _volumes()["mask"]

    def call():
        labels, count = components.label(m)
        return dict(labels=labels, count=count)

    def reference(out):
        want, k = ndi.label(host)
        assert int(out["count"]) == k and np.array_equal(out["labels"].cpu().numpy(), want.astype(np.int32))
    return call, reference


@case("components.label_65_chunks", ["ru3d_components_workspace_bytes"])
def _c_label_65():
    """(41, 47, 69) = 132963 voxels = 65 chunks of 2048: the layout's regions are rounded up to 256 bytes, so a count row
    too few in the query shows only where the row of 4-byte chunk counts begins a new 256-byte line, at 64 k + 1 chunks.
    Sparse blobs keep scipy quick"""
    shape = (41, 47, 69)
    rng = np.random.RandomState(65)
    host = ndi.binary_dilation(rng.rand(*shape) < 0.004, iterations=2) | (rng.rand(*shape) < 0.01)
    host[-1, -1, -1] = True
    m = _up(host.astype(np.uint8))

    def call():
        labels, count = components.label(m)
        return dict(labels=labels, count=count)

    def reference(out):
        want, k = ndi.label(host)
        assert int(out["count"]) == k > 65 and np.array_equal(out["labels"].cpu().numpy(), want.astype(np.int32))
    return call, reference


def _labelled():
    host = _volumes()["mask"]
    want, k = ndi.label(host)
    sizes = np.bincount(want.ravel(), minlength=k + 1)[1:]
    return host, want.astype(np.int32), k, sizes


@case("components.stats")
def _c_stats():
    host, lab, k, sizes = _labelled()
    d = _up(lab)

    def call():
        return dict(zip(("sizes", "boxes"), components.stats(d, k)))

    def reference(out):
        boxes = np.array([[s.start, s.stop] for obj in ndi.find_objects(lab) for s in obj]).reshape(k, 6)
        assert np.array_equal(out["sizes"].cpu().numpy(), sizes) and np.array_equal(out["boxes"].cpu().numpy(), boxes)
    return call, reference


def _filter(relabel):
    host, lab, k, sizes = _labelled()
    d, dsizes, dmask = _up(lab), _up(sizes.astype(np.int32)), _up(host.astype(np.uint8))
    keep = sizes >= 4

    def call():
        m = dmask.clone()
        out, kept = components.filter_small(d, k, dsizes, 4, mask=m, relabel=relabel)
        return dict(mask=m, kept=kept, **(dict(labels=out) if relabel else {}))

    def reference(out):
        survivors = host & np.concatenate(([False], keep))[lab]
        assert 0 < keep.sum() < k and int(out["kept"]) == int(keep.sum())
        assert np.array_equal(out["mask"].cpu().numpy().astype(bool), survivors)
        if relabel:                                   # renumbered in order: a second labelling of the survivors
            assert np.array_equal(out["labels"].cpu().numpy(), ndi.label(survivors)[0].astype(np.int32))
    return call, reference


case("components.filter_small", ["ru3d_filter_components_workspace_bytes"])(lambda: _filter(False))
case("components.filter_small_relabel", ["ru3d_filter_components_workspace_bytes"])(lambda: _filter(True))


# ---- distance.py (reference: the contract's brute force and numpy, tests/test_gpu_distance.py, equality)
@case("distance.edt_squared", ["ru3d_edt_workspace_bytes"])
def _d_edt():
    p, host = _pack(_volumes()["feat"]), _volumes()["feat"]

    def reference(out):
        assert np.array_equal(out["sq"].cpu().numpy(), _edt_brute(host))
    return (lambda: dict(sq=distance.edt_squared(p))), reference


@case("distance.surface")
def _d_surface():
    p, host = _pack(_volumes()["solid"]), _volumes()["solid"]

    def reference(out):
        assert np.array_equal(_bools(out["surface"]), host & ~ndi.binary_erosion(host))
    return (lambda: dict(surface=distance.surface(p))), reference


def _gather(capacity):
    host_sq, query = _edt_brute(_volumes()["feat"]), _volumes()["mask"]
    sq, q, n = _up(host_sq), _pack(query), int(query.sum())

    def call():
        if capacity is None:
            return dict(values=distance.gather(sq, q))
        values, count = distance.gather(sq, q, capacity=capacity)
        # the rule of gather(capacity=): the first min(count, capacity) values are valid, nothing is written beyond them
        return dict(values=values[:min(int(count.item()), capacity)], count=count)

    def reference(out):
        assert np.array_equal(out["values"].cpu().numpy(), host_sq[query][:capacity])
        assert capacity is None or int(out["count"]) == n
    return call, reference


case("distance.gather", ["ru3d_edt_gather_workspace_bytes"])(lambda: _gather(None))
case("distance.gather_capacity", ["ru3d_edt_gather_workspace_bytes"])(lambda: _gather(int(_volumes()["mask"].sum()) + 37))
case("distance.gather_capacity_too_small", ["ru3d_edt_gather_workspace_bytes"])(lambda: _gather(2049))


@case("distance.reduce", ["ru3d_edt_reduce_workspace_bytes"])
def _d_reduce():
    """the reduction behind the surface-distance metrics, over the first 6001 of 6030 gathered values"""
    v = _edt_brute(_volumes()["feat"]).ravel()
    n = v.size - 29
    values, count = _up(v), torch.tensor([n], dtype=torch.int64, device=DEV)

    def reference(out):
        got = out["red"].cpu().numpy()
        assert got[0] == n and got[1] == v[:n].max() and got[2] == (v[:n] <= 2.25).sum()
        assert got[3] == pytest.approx(np.sqrt(v[:n]).sum(), rel=1e-13)
    return (lambda: dict(red=distance.reduce(values, count, 2.25))), reference


# ---- skeleton.py (reference: the numpy twins of transform.py, tests/test_gpu_skeleton.py, equality)
@functools.lru_cache(maxsize=None)
def _skel():
    solid = _volumes()["solid"]
    skel, iterations = T._skeleton_numpy(solid)
    assert skel.any() and iterations > 1
    skel.setflags(write=False)
    return solid, skel, iterations


@case("skeleton.thin", ["ru3d_skeleton_workspace_bytes"])
def _s_thin():
    solid, want, iterations = _skel()
    p = _pack(solid)
    before = p.bits.clone()

    def call():
        skel, it = skeleton.thin(p, return_iterations=True)
        assert torch.equal(p.bits, before)
        return dict(skel=skel, iterations=it)

    def reference(out):
        assert np.array_equal(_bools(out["skel"]), want) and int(out["iterations"]) == iterations
    return call, reference


@case("skeleton.classify")
def _s_classify():
    _, skel, _ = _skel()
    p = _pack(skel)

    def call():
        ends, junctions, n, n_ends, n_junctions = skeleton.classify(p)
        return dict(ends=ends, junctions=junctions, counts=[n, n_ends, n_junctions])

    def reference(out):
        want = T._skeleton_classify_numpy(skel)
        assert out["counts"].tolist() == list(want[2:])
        assert np.array_equal(_bools(out["ends"]), want[0]) and np.array_equal(_bools(out["junctions"]), want[1])
    return call, reference


@case("skeleton.length")
def _s_length():
    """ru3d_skeleton_length has no query: its scratch is the 256 bytes of counters (SK_COUNTERS) the wrapper asks for"""
    _, skel, _ = _skel()
    p, spacing = _pack(skel), (0.75, 0.5, 3.0)

    def reference(out):
        assert float(out["length"]) == T._skeleton_length_numpy(skel, spacing) > 0
    return (lambda: dict(length=skeleton.length_device(p, spacing))), reference


@case("skeleton.overlap")
def _s_overlap():
    _, skel, _ = _skel()
    other = _volumes()["mask"]
    a, b = _pack(skel), _pack(other)

    def reference(out):
        assert out["counts"].tolist() == [int(skel.sum()), int(other.sum()), int((skel & other).sum())]
    return (lambda: dict(counts=skeleton.overlap_device(a, b))), reference


@case("skeleton.complement")
def _s_complement():
    solid = _volumes()["solid"]
    p = _pack(solid)

    def reference(out):
        assert np.array_equal(_bools(out["complement"]), ~solid)
    return (lambda: dict(complement=skeleton.complement(p))), reference


@case("skeleton.radii_squared", ["ru3d_edt_workspace_bytes", "ru3d_edt_gather_workspace_bytes"])
def _s_radii():
    solid, skel, _ = _skel()
    s, m = _pack(skel), _pack(solid)

    def reference(out):
        assert np.array_equal(out["sq"].cpu().numpy(), _edt_brute(~solid)[skel])
    return (lambda: dict(sq=skeleton.radii_squared(s, m))), reference


@case("skeleton.radius_stats")
def _s_radius_stats():
    solid, skel, _ = _skel()
    host = _edt_brute(~solid)[skel]
    sq = _up(host)

    def reference(out):
        assert tuple(out["stats"].tolist()) == tuple(float(v) for v in trainer._radius_stats_numpy(host))
    return (lambda: dict(stats=skeleton.radius_stats(sq))), reference


# ---- mesh.py through transform.extract_mesh (reference: its numpy route, tests/test_gpu_mesh.py, equality)
@case("mesh.extract_measure", ["ru3d_mesh_workspace_bytes", "ru3d_mesh_measure_workspace_bytes"])
def _m_mesh():
    host = _volumes()["mask"]
    d = _up(host)

    def call():
        m = T.extract_mesh(d, 0)
        return dict(corners=m.corners, vertices=m.vertices, faces=m.faces, neighbours=m.neighbours,
                    measure=mesh.measure(m.vertices, m.faces))

    def reference(out):
        want = T.extract_mesh(host, 0)
        for name in ("corners", "faces", "neighbours", "vertices"):
            assert np.array_equal(out[name].cpu().numpy(), getattr(want, name)), name
        assert out["measure"].tolist() == [float(len(want.faces) // 2), float(host.sum())]
    return call, reference


# ---- morphology.py (reference: scipy and numpy, tests/test_gpu_morphology.py, equality)
def _m_pack(op, value):
    host = _volumes()["pred"]
    d = _up(host)
    want = {"ne": host != value, "eq": host == value, "gt": host > value, "ge": host >= value}[op]

    def reference(out):
        assert np.array_equal(_bools(out["mask"]), want)
    return (lambda: dict(mask=morphology.pack(d, op, value))), reference


case("morphology.pack_ne")(lambda: _m_pack("ne", 0))
case("morphology.pack_ge")(lambda: _m_pack("ge", 3))


@case("morphology.unpack")
def _m_unpack():
    host = _volumes()["mask"]
    p = _pack(host)

    def reference(out):
        assert np.array_equal(out["volume"].cpu().numpy(), host.astype(np.uint8) * 7)
    return (lambda: dict(volume=morphology.unpack(p, 7))), reference


def _m_binary(name):
    host = _volumes()["solid"] | (_volumes()["feat"])
    p = _pack(host)
    fn = {"erode": ndi.binary_erosion, "dilate": ndi.binary_dilation, "open": ndi.binary_opening,
          "close": ndi.binary_closing}[name]

    def reference(out):
        assert np.array_equal(_bools(out["mask"]), fn(host, iterations=2))
    return (lambda: dict(mask=getattr(morphology, name)(p, iterations=2))), reference


for _name in ("erode", "dilate", "open", "close"):
    case("morphology." + _name)(functools.partial(_m_binary, _name))


@case("morphology.confusion")
def _m_confusion():
    pred, label = _volumes()["pred"], _volumes()["label"]
    dp, dl = _up(pred), _up(label)

    def reference(out):
        c = 3
        want = np.zeros((c + 1, c + 1), np.int64)
        np.add.at(want, (np.minimum(label, c).ravel(), np.minimum(pred, c).ravel()), 1)
        assert np.array_equal(out["table"].cpu().numpy(), want)
    return (lambda: dict(table=morphology.confusion(dp, dl, 3))), reference


# ---- visualize.py's surface renderer (reference: its numpy route, tests/test_gpu_visualize.py, equality).  The renderer
# allocates its scratch itself (_Prepared.ws, torch.empty of the queried size): the stand-in for torch.empty hands it the
# hostile one.  Both entry points check the same figure; the short one meets the prepare call, which comes first
def _render_operands():
    volume = np.zeros(VOL, np.uint8)
    volume[_volumes()["solid"]] = 1
    volume[3:6, 4:7, 60:66] = 2
    table = V.colour_table(alpha={1: 0.5})
    view = V.fit_view(([0, 0, 0], list(VOL)), (1.0, 1.0, 2.0), 33, 21, 24)
    return volume, table, view


@case("visualize.surface_prepare", ["ru3d_render_surface_workspace_bytes"], kind="own_scratch")
def _v_prepare():
    volume, table, _ = _render_operands()
    d = _up(volume)

    def reference(out):
        assert np.array_equal(out["bricks"].numpy(), V._bricks_numpy(volume, table))
    return (lambda: dict(bricks=V._Prepared(d, table).bricks)), reference


@case("visualize.surface_render", ["ru3d_render_surface_workspace_bytes"], kind="own_scratch")
def _v_render():
    volume, table, view = _render_operands()
    d = _up(volume)

    def call():
        rgb, depth = V.cast_device(V._Prepared(d, table), view, 24, 24)
        return dict(rgb=rgb, depth=depth)

    def reference(out):
        rgb, depth = V.cast_numpy(volume, table, view, 24, 24)
        assert (depth >= 0).any()
        assert np.array_equal(out["depth"].numpy(), depth) and np.array_equal(out["rgb"].numpy(), rgb)
    return call, reference


# ---- prepare.py (reference: numpy, tests/test_gpu_prepare.py, equality; mean and std to 1e-12)
@functools.lru_cache(maxsize=None)
def _image():
    rng = np.random.RandomState(9)
    img = rng.standard_normal(VOL + (2,)).astype(np.float32)
    img.setflags(write=False)
    return img


@case("prepare.threshold_bbox")
def _p_bbox():
    img = _image()
    d = _up(img)

    def call():
        box, n = prepare.threshold_bbox(d, 2.0)
        return dict(box=box, n=n)

    def reference(out):
        idx = np.where((img > 2.0).any(axis=3))
        assert int(out["n"]) == len(idx[0]) > 0
        assert np.array_equal(out["box"].numpy(), np.array([[i.min(), i.max()] for i in idx]))
    return call, reference


@case("prepare.masked_sample", ["ru3d_masked_sample_workspace_bytes"])
def _p_sample():
    img, label = _image(), _volumes()["label"]
    d, dl = _up(img), _up(label)

    def reference(out):
        assert np.array_equal(out["sample"].cpu().numpy(), img[..., 1][label > 0][::3])
    return (lambda: dict(sample=prepare.masked_sample(d, dl, 1, stride=3))), reference


@case("prepare.order_statistics", ["ru3d_order_stats_workspace_bytes"])
def _p_order():
    v = _image().ravel()
    d, ranks = _up(v), [0, 5, v.size // 2, v.size - 1]

    def reference(out):
        assert np.array_equal(out["picked"].numpy(), np.sort(v)[ranks])
    return (lambda: dict(picked=prepare.order_statistics(d, ranks))), reference


@case("prepare.moments", ["ru3d_moments_workspace_bytes"])
def _p_moments():
    v = _image().ravel()
    d = _up(v)

    def reference(out):
        n, lo, hi, mean, std = out["moments"].tolist()
        assert (n, lo, hi) == (v.size, float(v.min()), float(v.max()))
        v64 = v.astype(np.float64)
        assert mean == pytest.approx(v64.mean(), rel=1e-12, abs=1e-15) and std == pytest.approx(v64.std(), rel=1e-12)
    return (lambda: dict(moments=prepare.moments(d))), reference


# ---- augment.py, degrade.py (reference: the numpy twins of transform.py and degrade.py; tolerances of
# tests/test_gpu_oversample.py, test_gpu_spatial.py, test_gpu_augment_degrade.py)
@functools.lru_cache(maxsize=None)
def _patient():
    rng = np.random.RandomState(80)
    g = np.meshgrid(*[np.linspace(-1, 1, s, dtype=np.float32) for s in CASE_SHAPE], indexing="ij")
    img = np.stack([np.sin((4 + c) * g[0]) * np.cos(3 * g[1] + c) + g[2] ** 2 + 0.05 * rng.randn(*CASE_SHAPE)
                    for c in range(CHANNELS)], axis=-1).astype(np.float32)
    lab = np.zeros(CASE_SHAPE, dtype=np.uint8)
    lab[np.sqrt(g[0] ** 2 + (1.2 * g[1]) ** 2 + g[2] ** 2) < 0.8] = 1
    lab[np.sqrt((g[0] - 0.2) ** 2 + g[1] ** 2 + g[2] ** 2) < 0.35] = 2
    lab[np.sqrt((g[0] + 0.6) ** 2 + (g[1] - 0.5) ** 2 + (g[2] + 0.5) ** 2) < 0.2] = 3
    img.setflags(write=False), lab.setflags(write=False)
    return img, lab, augment.DeviceCase(img, lab, DEV)


SPATIAL = dict(rotation=((-0.3, 0.3), (-0.1, 0.1), (0, 0.2)), elastic_spacing=8, elastic_magnitude=(0, 2))


def _sampler(spatial):
    """DeviceAugment.sample itself, seeded anew in every call: the same draws, and the presence mask (torch.empty,
    cleared by ru3d_augment_label_presence's memset, read by the patch kernel), the lattice upload and the outputs are
    allocated inside the call.  The presence kernel is launched ahead of the one ask (AHEAD below).  The label has two
    classes: the patch kernel takes the highest set bit of the mask for the class count, and below three classes it
    interpolates and truncates where otherwise it takes the heaviest class - so bits left in an uncleared mask change
    the labels of the patch (with four classes they would change nothing)"""
    img, lab4, _ = _patient()
    lab = (lab4 > 0).astype(np.uint8)
    dcase = augment.DeviceCase(img, lab, DEV)
    kw = dict(scale=0.1, crop_size=list(PATCH), crop_mode="random", **(SPATIAL if spatial else {}))
    aug = augment.DeviceAugment(**kw)

    def call():
        np.random.seed(31)
        image, label = aug.sample(dcase)
        return dict(image=image, label=label)

    def reference(out):
        crop = T.RandomSpatialCrop(0.1, list(PATCH), crop_mode="random", **SPATIAL) if spatial else \
            T.RandomRescaleCrop(0.1, list(PATCH), crop_mode="random")
        np.random.seed(31)
        c = crop({"image": img.copy(), "label": lab.copy()})
        image, label = c["image"], c["label"]
        for axis in range(3):
            if np.random.uniform() < 0.5:
                image, label = np.flip(image, axis).copy(), np.flip(label, axis).copy()
        for op in (T.adjust_contrast, T.adjust_brightness, T.adjust_gamma):
            image = op(image, np.random.uniform(0.9, 1.1))
        want = np.moveaxis(image, -1, 0)
        differ = int((out["label"].cpu().numpy() != label.astype(np.int64)).sum())
        err = float(np.abs(out["image"].cpu().numpy() - want).max())
        print("sampler spatial=%s: %d label voxels differ, max |image difference| %.3g" % (spatial, differ, err))
        if spatial:         # tests/test_gpu_spatial.py: at most 8 label voxels on a tie of the trilinear weights
            assert differ <= 8 and err <= 2e-5 * max(1.0, float(np.abs(want).max()))
        else:               # tests/test_gpu_oversample.py
            assert differ == 0 and err <= 2e-5
    return call, reference


case("augment.sample", ["ru3d_augment_workspace_bytes"])(lambda: _sampler(False))
case("augment.sample_rotation_elastic", ["ru3d_augment_workspace_bytes"])(lambda: _sampler(True))


@case("augment.class_index", ["ru3d_class_index_workspace_bytes"])
def _a_index():
    _, lab, _ = _patient()
    d, m = _up(lab), 300

    def call():
        index = augment.ClassIndex(d, m)
        return dict(counts=index.counts, boxes=index.boxes, table=index.device_locations)

    def reference(out):
        counts, boxes, rows = T.class_locations(lab, m)
        table = np.full((32, m), -1, dtype=np.int32)
        for c, row in enumerate(rows):
            table[c, :len(row)] = row
        assert counts[3] > 0 and counts[1] > m
        assert np.array_equal(out["counts"].numpy(), counts) and np.array_equal(out["boxes"].numpy(), boxes)
        assert np.array_equal(out["table"].cpu().numpy(), table)            # every row, the -1 padding included
    return call, reference


@case("degrade.chain", ["ru3d_augment_workspace_bytes", "ru3d_augment_degrade_workspace_bytes"], kind="joint_ask")
def _g_chain():
    rng = np.random.RandomState(70)
    img = rng.standard_normal(PATCH + (CHANNELS,)).astype(np.float32)
    d = _up(img)
    chain = {"noise": (0.07, (1234567, 7654321)), "blur": 1.0, "low_res": 0.6}

    def reference(out):
        first = np.moveaxis(img, -1, 0)
        after_noise = degrade.gaussian_noise(first, *chain["noise"])
        after_blur = degrade.gaussian_blur(after_noise, chain["blur"])
        want = np.moveaxis(degrade.simulate_low_resolution(after_blur, chain["low_res"]), 0, -1)
        a, b = float(np.abs(after_noise).max()), float(np.abs(after_blur).max())
        bound = 1.4 * (EPS * a + 3 * EPS * a + EPS * b)        # the chain's bound of test_gpu_augment_degrade.py
        err = float(np.abs(out["image"].cpu().numpy().astype(np.float64) - want).max())
        print("degrade chain: max error %.3g, bound %.3g" % (err, bound))
        assert err <= bound
    return (lambda: dict(image=degrade.apply_device(d, chain))), reference


# ---- loss.py: the functional pieces
@case("loss.dice")
def _l_dice():
    """the functional dice: ru3d_tversky has no query; the wrapper asks for its block rows"""
    g = torch.Generator().manual_seed(5)
    p = torch.rand((2,) + LOSS_SPATIAL, generator=g)
    t = (torch.rand((2,) + LOSS_SPATIAL, generator=g) < 0.3).float()
    dp, dt = p.to(DEV), t.to(DEV)

    def reference(out):
        want = float(L.dice(p.double(), t.double(), 0.3, 0.7))
        assert abs(float(out["dice"]) - want) <= VALUE_TOL * max(1.0, abs(want))
    return (lambda: dict(dice=L.dice(dp, dt, 0.3, 0.7))), reference


def _grad_check(got, ref, floor, what):
    got = got.detach().to("cpu", torch.float64)
    assert got.shape == ref.shape and bool(torch.isfinite(got).all()), what
    tol = GRAD_REL * ref.abs() + floor * float(ref.abs().max())
    worst = float(((got - ref).abs() / tol.clamp_min(1e-300)).max())
    print("%s: worst gradient element %.3g of its bound (floor %.3g)" % (what, worst, floor))
    assert worst <= 1.0, what


def _host_floor(fn, x, ref_g):
    """the floor rule of tests/test_gpu_cldice.py and test_gpu_boundary.py: twice what the same chain in float32 on the
    host misses the float64 reference by (worst element over max|ref|), rounded up to two digits"""
    z = x.clone().float().requires_grad_(True)
    fn(z).backward()
    miss = float((z.grad.double() - ref_g).abs().max() / ref_g.abs().max())
    digits = 10.0 ** (math.floor(math.log10(max(miss, 1e-12))) - 1)
    return 2.0 * math.ceil(miss / digits) * digits


@case("loss.soft_skeleton", ["ru3d_cldice_workspace_bytes"])
def _l_skeleton():
    g = torch.Generator().manual_seed(3)
    p = torch.rand((2, 2) + LOSS_SPATIAL, generator=g)
    up = torch.randn((2, 2) + LOSS_SPATIAL, generator=g)
    dp, dup = p.to(DEV), up.to(DEV)

    def call():
        x = dp.clone().requires_grad_(True)
        s = L.soft_skeleton(x, 2)
        s.backward(dup)
        return dict(skeleton=s, grad=x.grad)

    def reference(out):
        z = p.double().requires_grad_(True)
        want = L._soft_skeleton_host(z, 2)
        want.backward(up.double())
        # values: 2^-23 per level with a positive delta (forward_bound of tests/test_gpu_cldice.py), three levels here
        assert float((out["skeleton"].cpu().double() - want.detach()).abs().max()) <= 3 * 2.0 ** -23
        floor = _host_floor(lambda t: (L._soft_skeleton_host(t, 2) * up).sum(), p, z.grad)
        _grad_check(out["grad"], z.grad, floor, "soft_skeleton")
    return call, reference


def _l_sdm(squared):
    y = LOSS_LABELS()
    dy = y.to(DEV)

    def reference(out):
        want = L._signed_squares_host(y, (1, 2))
        assert torch.equal(out["map"].cpu(), want if squared else L._phi_of_squares(want))
    return (lambda: dict(map=L.signed_distance_map(dy, 3, squared=squared))), reference


case("loss.signed_distance_map", ["ru3d_boundary_workspace_bytes"])(lambda: _l_sdm(False))
case("loss.signed_distance_map_squared", ["ru3d_boundary_workspace_bytes"])(lambda: _l_sdm(True))


# ---- loss.py: the fifteen criteria of test_gpu_loss_contract.CRITERIA, forward and backward
@functools.lru_cache(maxsize=None)
def LOSS_LABELS():
    """blobs of classes 1 and 2 in a background: every class has an inside and a boundary in both samples"""
    g = np.meshgrid(*[np.linspace(-1, 1, s) for s in LOSS_SPATIAL], indexing="ij")
    y = np.zeros((2,) + LOSS_SPATIAL, dtype=np.int64)
    for n, shift in enumerate((0.0, 0.25)):
        y[n][np.sqrt((g[0] - shift) ** 2 + g[1] ** 2 + g[2] ** 2) < 0.7] = 1
        y[n][np.sqrt((g[0] + 0.2) ** 2 + (g[1] - shift) ** 2 + (g[2] - 0.3) ** 2) < 0.3] = 2
    return torch.from_numpy(y)


@functools.lru_cache(maxsize=None)
def _loss_operands(name):
    _, c, ds = LC.CRITERIA[name]
    g = torch.Generator().manual_seed(7 + len(name))
    xs = [2.0 * torch.randn((2, c) + shape, generator=g) for shape in ([LOSS_SPATIAL, LOSS_LEVEL1] if ds else [LOSS_SPATIAL])]
    return xs, LOSS_LABELS()


def _loss_twin(name, zs, t):
    """the float64 (or float32) host twin of a criterion on host logits `zs` (a list: the levels) and labels t"""
    crit, z = LC.CRITERIA[name][0](), zs[0]

    def hybird(c):
        return L._region_loss_host(N.LOSS_HYBIRD, z, t, c.gamma, c.weight_v, c.alpha, c.beta, c.smooth)
    if name in ("Dice", "DiceLoss", "FocalLoss", "HybirdLoss"):
        return L._region_loss_host(crit._kind, z, t, getattr(crit, "gamma", 2.0), crit.weight_v, getattr(crit, "alpha", 0.5),
                                   getattr(crit, "beta", 0.5), getattr(crit, "smooth", 1e-7))
    if name == "SoftClDiceLoss":
        return L._soft_cldice_host(z, t, crit.iterations, crit.classes, crit.weight_v, crit.smooth)
    if name == "HybirdClDiceLoss":
        lam = crit.cl_weight
        return (1.0 - lam) * hybird(crit) + lam * L._soft_cldice_host(z, t, crit.iterations, crit.classes, crit.weight_v,
                                                                     crit.cl_smooth)
    if name == "BoundaryLoss":
        return L._boundary_host(z, t, crit.classes, crit.weight_v)
    if name == "HybirdBoundaryLoss":
        a = float(crit.boundary_weight)
        return (1.0 - a) * hybird(crit) + a * L._boundary_host(z, t, crit.classes, crit.weight_v)
    return crit(zs if LC.CRITERIA[name][2] else z, t)       # deep supervision, groups: the modules' own host route


LOSS_QUERIES = {
    "SoftClDiceLoss": ["ru3d_cldice_workspace_bytes", "ru3d_cldice_state_bytes"],
    "HybirdClDiceLoss": ["ru3d_loss_workspace_bytes", "ru3d_loss_state_bytes", "ru3d_cldice_workspace_bytes",
                         "ru3d_cldice_state_bytes"],
    "BoundaryLoss": ["ru3d_boundary_workspace_bytes", "ru3d_boundary_state_bytes"],
    "HybirdBoundaryLoss": ["ru3d_loss_workspace_bytes", "ru3d_loss_state_bytes", "ru3d_boundary_workspace_bytes",
                           "ru3d_boundary_state_bytes"],
    "DeepSupervisionLoss": ["ru3d_ds_loss_workspace_bytes", "ru3d_ds_state_bytes"],
    "TopKLoss": ["ru3d_topk_loss_workspace_bytes", "ru3d_topk_loss_state_bytes"],
    "HybirdTopKLoss": ["ru3d_topk_loss_workspace_bytes", "ru3d_topk_loss_state_bytes"],
}
for _name in LC.NAMES:
    LOSS_QUERIES.setdefault(_name, ["ru3d_group_loss_workspace_bytes", "ru3d_group_loss_state_bytes"]
                            if _name.startswith("Group") else ["ru3d_loss_workspace_bytes", "ru3d_loss_state_bytes"])


def _criterion(name):
    xs, y = _loss_operands(name)
    dxs, dy = [x.to(DEV) for x in xs], y.to(DEV)
    ds = LC.CRITERIA[name][2]

    def call(labels=None, check_labels=True):
        crit = LC.CRITERIA[name][0]()
        crit.check_labels = check_labels
        lv = [x.clone().requires_grad_(True) for x in dxs]
        v = crit(lv if ds else lv[0], dy if labels is None else labels)
        v.backward()
        return dict(value=v, **{"grad%d" % i: x.grad for i, x in enumerate(lv)})

    def reference(out):
        zs = [x.double().requires_grad_(True) for x in xs]
        if name in ("TopKLoss", "HybirdTopKLoss"):          # the references of tests/test_gpu_topk.py, near voxels left out
            ref_v, ref_g, near, _ = TK.reference_topk(xs[0], y, 10)
            if name == "HybirdTopKLoss":
                dice_v, dice_g = TK.reference_dice(xs[0], y)
                ref_v, ref_g = ref_v + dice_v, ref_g + dice_g
            TK.assert_value(out["value"], ref_v, name)
            n, c = xs[0].shape[:2]
            TK.assert_grad(out["grad0"].reshape(n, c, -1), ref_g.reshape(n, c, -1), name, near)
            return
        want = _loss_twin(name, zs, y)
        want.backward()
        got, ref_v = float(out["value"]), float(want.detach())
        print("%s: value %.9g, float64 %.9g" % (name, got, ref_v))
        assert abs(got - ref_v) <= VALUE_TOL * max(1.0, abs(ref_v))
        floor = GRAD_FLOOR
        if "ClDice" in name or "Boundary" in name:
            floor = _host_floor(lambda t: _loss_twin(name, [t], y), xs[0], zs[0].grad)
        for i, z in enumerate(zs):
            _grad_check(out["grad%d" % i], z.grad, floor, "%s level %d" % (name, i))
    return call, reference


for _name in LC.NAMES:
    case("loss." + _name, LOSS_QUERIES[_name], kind="loss")(functools.partial(_criterion, _name))


# ---- the select of the top-k losses alone: no wrapper, the direct call of tests/test_gpu_topk.py::select with the scratch
# taken from N.workspace, as every wrapper takes it
@case("topk.select", ["ru3d_topk_select_workspace_bytes"])
def _t_select():
    v = np.abs(np.random.RandomState(4).standard_normal(6001)).astype(np.float32)
    v[::3] = 0.0
    d, k = _up(v), 600

    def call():
        res = torch.empty(32, dtype=torch.uint8, device=DEV)
        ws = N.workspace(N.lib.ru3d_topk_select_workspace_bytes(d.numel()), DEV)
        N.note_device(DEV)
        N.check(N.lib.ru3d_topk_select(N.ptr(d), d.numel(), k, N.ptr(res), N.ptr(ws), ws.numel(), N.stream()), "topk_select")
        # the result block is 4 bytes of tau, 4 of padding, two int64 counts and a float64 sum: the padding is not written
        return dict(tau=res[:4].clone(), rest=res[8:].clone())

    def reference(out):
        tau = np.partition(v, v.size - k)[v.size - k]
        above = v[v > tau].astype(np.float64)
        gt, eq = out["rest"][:16].cpu().numpy().view(np.int64)
        total = float(out["rest"][16:].cpu().numpy().view(np.float64)[0])
        assert out["tau"].cpu().numpy().view(np.float32)[0] == tau and gt == above.size and eq == int((v == tau).sum())
        assert abs(total - math.fsum(above.tolist())) <= v.size * 2.0 ** -53 * math.fsum(above.tolist())
    return call, reference


# ---- propagation and hole filling (reference: scipy, tests/test_gpu_postprocess.py, equality).  No scratch: the flood's
# counters are a torch.empty vector, which the stand-in fills.  last_rounds is an output: a leftover byte must not move it
@case("morphology.propagate")
def _m_propagate():
    """(20, 10, 67), two tiles of the flood along x: the corridor of contract_inputs.flood_zigzag takes more rounds
    than the first batch has"""
    seed, allowed, _, _ = CI.flood_zigzag()
    s, a = _pack(seed), _pack(allowed)
    before = s.bits.clone(), a.bits.clone()

    def call():
        reach = morphology.propagate(s, a, None, 0)
        assert torch.equal(s.bits, before[0]) and torch.equal(a.bits, before[1])
        return dict(reach=reach, rounds=morphology.last_rounds)

    def reference(out):
        assert int(out["rounds"]) > CI.FLOOD_FIRST_BATCH, "one batch of rounds: %d" % int(out["rounds"])
        assert np.array_equal(_bools(out["reach"], CI.FLOOD_SHAPE), ndi.binary_propagation(seed, mask=allowed))
    return call, reference


@case("morphology.propagate_cube_border")
def _m_propagate_border():
    """allowed=None: the complement of an empty mask, inverted on load; the full cube, the outside set"""
    seed = CI.flood_cube_seed()
    s = _pack(seed)

    def call():
        return dict(reach=morphology.propagate(s, None, CI.CUBE, 1), rounds=morphology.last_rounds)

    def reference(out):
        want = ndi.binary_propagation(seed, structure=CI.CUBE, border_value=1)
        assert want.all() and np.array_equal(_bools(out["reach"]), want)
    return call, reference


@case("morphology.fill_holes")
def _m_fill_holes():
    solid, tunnel = CI.solid_with_cavities()
    p = _pack(solid)

    def call():
        return dict(filled=morphology.fill_holes(p), rounds=morphology.last_rounds)

    def reference(out):
        got = _bools(out["filled"])
        assert np.array_equal(got, ndi.binary_fill_holes(solid))
        assert (got & ~solid).sum() > 0 and not got[tunnel].any()          # cavities filled, the tunnel not
    return call, reference


# ---- components.keep_largest (reference: the numpy twin of tests/postprocess_cases.py, equality)
def _keep(relabel):
    host, lab, k, sizes = CI.keep_volume()
    d, dsizes, dmask = _up(lab), _up(sizes.astype(np.int32)), _up(host.astype(np.uint8))

    def call():
        m = dmask.clone()
        out, kept = components.keep_largest(d, k, dsizes, k=2, mask=m, relabel=relabel)
        return dict(mask=m, kept=kept, **(dict(labels=out) if relabel else {}))

    def reference(out):
        want_mask, want_labels = CI.keep_largest_numpy(host, 2)
        assert int(out["kept"]) == 2 and np.array_equal(out["mask"].cpu().numpy().astype(bool), want_mask)
        if relabel:
            assert np.array_equal(out["labels"].cpu().numpy(), want_labels.astype(np.int32))
    return call, reference


case("components.keep_largest", ["ru3d_filter_components_workspace_bytes"])(lambda: _keep(False))
case("components.keep_largest_relabel", ["ru3d_filter_components_workspace_bytes"])(lambda: _keep(True))


# ---- morphometry.py (reference: its numpy route, tests/test_gpu_morphometry.py: equality; extents to the rounding of a
# four-term sum).  No scratch: every table is a torch.empty of the wrapper.  Plain names: the int32 components of the
# speckle mask (id_bytes 4); _u8: a uint8 class volume (id_bytes 1)
def _mm(id_bytes):
    ids, count, other, num_other = CI.morphometry_ids(id_bytes)
    return ids, count, other, num_other, _up(ids), (None if other is None else _up(other))


def _mm_moments(id_bytes):
    ids, count, _, _, d, _ = _mm(id_bytes)

    def reference(out):
        assert np.array_equal(out["moments"].cpu().numpy(), morphometry.moments(ids, count))
    return (lambda: dict(moments=morphometry.moments(d, count))), reference


def _mm_faces(id_bytes):
    """int32 ids against `other`; the uint8 volume in class mode"""
    ids, count, other, num_other, d, o = _mm(id_bytes)

    def reference(out):
        assert np.array_equal(out["faces"].cpu().numpy(), morphometry.faces(ids, count, other, num_other))
    return (lambda: dict(faces=morphometry.faces(d, count, o, num_other))), reference


def _mm_extents(id_bytes):
    ids, count, _, _, d, _ = _mm(id_bytes)
    frames = CI.morphometry_frames(count)

    def reference(out):
        got, want = out["extents"].cpu().numpy(), morphometry.extents(ids, count, frames)
        # extent_tolerance of tests/test_gpu_morphometry.py: 4 u (|ax x| + |ay y| + |az z| + |b|), the largest of an id
        tol = np.zeros((count, 3))
        lin, k = morphometry._valid(ids, count)
        x, y, z = (c.astype(np.float64)[:, None] for c in morphometry._xyz(lin, ids.shape))
        fk = np.abs(frames)[k - 1]
        np.maximum.at(tol, k - 1, fk[:, :, 0] * x + fk[:, :, 1] * y + fk[:, :, 2] * z + fk[:, :, 3])
        tol *= 4 * 2.0 ** -53
        finite = np.isfinite(want)
        assert not finite.all() and np.array_equal(np.isfinite(got), finite) and np.array_equal(got[~finite], want[~finite])
        err = np.abs(np.where(finite, got, 0.0) - np.where(finite, want, 0.0))
        print("extents id_bytes=%d: worst error / bound %.3g" % (id_bytes, (err / np.maximum(tol[:, :, None], 1e-300)).max()))
        assert np.all(err <= tol[:, :, None]) and np.array_equal(got[:, 0], want[:, 0])
    return (lambda: dict(extents=morphometry.extents(d, count, frames))), reference


def _sorted_groups(cand, starts, counts):
    groups = [np.sort(cand[s:s + c]) for s, c in zip(starts.tolist(), counts.tolist())]
    return np.concatenate(groups) if groups else cand


def _mm_candidates(id_bytes):
    """the device leaves the order inside a group undefined: the case returns every group sorted (sorted_groups of
    tests/test_gpu_morphometry.py)"""
    ids, count, _, _, d, _ = _mm(id_bytes)

    def call():
        cand, starts, counts = morphometry.candidates(d, count)
        return dict(cand=_sorted_groups(cand.cpu().numpy(), starts.cpu(), counts.cpu()), starts=starts, counts=counts)

    def reference(out):
        cand, starts, counts = morphometry.candidates(ids, count)
        assert np.array_equal(out["counts"].cpu().numpy(), counts) and np.array_equal(out["starts"].cpu().numpy(), starts)
        assert np.array_equal(out["cand"].numpy(), _sorted_groups(cand, starts, counts))
    return call, reference


def _mm_feret(id_bytes):
    """voxel units: every term of d^2 is a small integer, so the float64 sums are exact and d^2 is held with ==; the
    pair as tests/test_gpu_morphometry.py holds it: two voxels of the id that give d^2 back"""
    ids, count, _, _, d, _ = _mm(id_bytes)

    def call():
        d2, pair = morphometry.feret(d, count)
        return dict(d2=d2, pair=pair)

    def reference(out):
        d2, pair = out["d2"].cpu().numpy(), out["pair"].cpu().numpy()
        want, _ = morphometry.feret(ids, count)
        assert np.array_equal(d2, want)
        n = morphometry.moments(ids, count)[:, 0]
        assert np.array_equal(d2 < 0, n == 0) and np.all(d2[n == 1] == 0.0)
        for k in range(count):
            if n[k] == 0:
                assert pair[k].tolist() == [-1] * 6
            else:
                assert ids[tuple(pair[k, :3])] == k + 1 and ids[tuple(pair[k, 3:])] == k + 1
                assert float(((pair[k, :3] - pair[k, 3:]).astype(np.int64) ** 2).sum()) == d2[k]
    return call, reference


for _name, _fn in (("moments", _mm_moments), ("faces", _mm_faces), ("extents", _mm_extents),
                   ("candidates", _mm_candidates), ("feret", _mm_feret)):
    case("morphometry." + _name)(functools.partial(_fn, 4))
    case("morphometry.%s_u8" % _name)(functools.partial(_fn, 1))


# ---- skeleton.graph and prune (reference: the numpy twins of transform.py, tests/test_gpu_skeleton_graph.py, equality
# with nan equal to nan).  The host tables come back as numpy
GRAPH_TABLES = ('n', 'nodes', 'branches', 'node_table', 'branch_table', 'length', 'chord', 'tortuosity')
GRAPH_RADII = ('radius_min', 'radius_mean', 'radius_max')


def _graph(with_mask, regrow=False):
    skel = CI.wire_tree()
    p = _pack(skel)
    m = _pack(CI.wire_lumen()) if with_mask else None
    sampling = CI.SAMPLING if with_mask else None

    def call():
        if not regrow:
            return dict(skeleton.graph(p, m, sampling))
        saved = dict(skeleton._ids_capacity)
        skeleton._ids_capacity[p.device] = CI.FORCED_IDS_CAPACITY          # below n: the ids buffer grows, a second labelling
        try:
            return dict(skeleton.graph(p, m, sampling), capacity=skeleton._ids_capacity[p.device])
        finally:
            skeleton._ids_capacity.clear()
            skeleton._ids_capacity.update(saved)

    def reference(out):
        sq = trainer._radii_squared_numpy(skel, CI.wire_lumen(), CI.SAMPLING) if with_mask else None
        want = T._skeleton_graph_numpy(skel, sq, CI.SAMPLING if with_mask else (1.0, 1.0, 1.0))
        keys = GRAPH_TABLES + (GRAPH_RADII if with_mask else ())
        assert set(out) == set(want) | ({"capacity"} if regrow else set())
        assert out["ids"].dtype == torch.int32 and np.array_equal(out["ids"].cpu().numpy(), want["ids"])
        for k in keys:
            got = out[k].numpy()
            assert same(got if got.ndim else got.item(), want[k]), k
        if regrow:
            assert CI.FORCED_IDS_CAPACITY < want["n"] <= int(out["capacity"]) == 1 << (want["n"] - 1).bit_length()
    return call, reference


case("skeleton.graph", ["ru3d_skeleton_workspace_bytes"])(lambda: _graph(False))
case("skeleton.graph_radii", ["ru3d_skeleton_workspace_bytes", "ru3d_edt_workspace_bytes"])(lambda: _graph(True))
case("skeleton.graph_regrow", ["ru3d_skeleton_workspace_bytes"])(lambda: _graph(False, regrow=True))


@case("skeleton.prune", ["ru3d_skeleton_workspace_bytes"])
def _s_prune():
    skel = CI.wire_tree()
    p = _pack(skel)
    before = p.bits.clone()

    def call():
        pruned, rounds = skeleton.prune(p, CI.PRUNE_MIN_LENGTH)
        assert torch.equal(p.bits, before)
        return dict(pruned=pruned, rounds=rounds)

    def reference(out):
        want, rounds = T._skeleton_prune_numpy(skel, CI.PRUNE_MIN_LENGTH)
        assert int(out["rounds"]) == rounds >= 3 and np.array_equal(_bools(out["pruned"]), want)
    return call, reference


# ---- territory.py (reference: the numpy twins of transform.py, tests/test_gpu_territory.py, equality)
def _t_nearest(return_sq):
    """return_sq=False asks for 8 X Y Z bytes more: the values then live in the scratch"""
    host = CI.sites()[0]
    s = _pack(host)

    def call():
        index, sq = territory.nearest(s, CI.SAMPLING, return_sq=return_sq)
        assert return_sq or sq is None
        return dict(index=index, **(dict(sq=sq) if return_sq else {}))

    def reference(out):
        index, sq = T._nearest_site_numpy(host, CI.SAMPLING)
        assert np.array_equal(out["index"].cpu().numpy(), index)
        assert not return_sq or np.array_equal(out["sq"].cpu().numpy(), sq)
    return call, reference


case("territory.nearest", ["ru3d_edt_workspace_bytes"])(lambda: _t_nearest(True))
case("territory.nearest_index_only", ["ru3d_edt_workspace_bytes"])(lambda: _t_nearest(False))


def _t_assign(with_region):
    host, site_ids, _, region, _ = CI.sites()
    index, want = CI.site_labels(with_region)
    s, ids, idx = _pack(host), _up(site_ids), _up(index)
    r = _pack(region) if with_region else None

    def reference(out):
        assert np.array_equal(out["labels"].cpu().numpy(), want)
    return (lambda: dict(labels=territory.assign(s, ids, idx, r))), reference


case("territory.assign", ["ru3d_skeleton_workspace_bytes"])(lambda: _t_assign(False))
case("territory.assign_region", ["ru3d_skeleton_workspace_bytes"])(lambda: _t_assign(True))


def _t_tally(K):
    """ru3d_territory_tally has no query: its scratch is the 256 bytes of the error word (TR_TALLY_WORKSPACE).  K = 6:
    the counters of a workgroup in LDS; K = 4000: (K + 1) * 3 cells are beyond LDS, 64-bit atomics on the table"""
    _, _, _, region, other = CI.sites()
    labels = CI.site_labels(True)[1]
    d, o, r = _up(labels), _up(other), _pack(region)

    def reference(out):
        assert np.array_equal(out["table"].cpu().numpy(), T._territory_tally_numpy(labels, K, other, 2, region))
    return (lambda: dict(table=territory.tally(d, K, o, 2, r))), reference


case("territory.tally")(lambda: _t_tally(CI.sites()[2]))
case("territory.tally_beyond_lds")(lambda: _t_tally(CI.TALLY_BEYOND_LDS))


def _t_partition(metric):
    """the composed driver on the wire tree inside its organ: nearest + assign + tally, or unpack + grow + tally"""
    skel, g, region, vessel, other = CI.organ()
    p, r, v, o = _pack(skel), _pack(region), _pack(vessel), _up(other)
    dg = dict(ids=_up(g["ids"]), branches=g["branches"], nodes=g["nodes"])

    def call():
        table, labels = territory.partition(p, dg, r, CI.SAMPLING, o, 1, metric=metric, vessel=v)
        return dict(table=table, labels=labels)

    def reference(out):
        site_ids, K = territory.branch_sites(g)
        if metric == "euclidean":
            index, _ = T._nearest_site_numpy(skel, CI.SAMPLING)
            labels = T._site_assign_numpy(skel, site_ids, index, region)
        else:
            seeds = np.zeros(VOL, dtype=np.int32)
            seeds[skel] = site_ids
            labels = np.where(region, CI.grow_twin(seeds, region | vessel, 3)[1], 0).astype(np.int32)
        assert (labels[region] > 0).any()
        assert np.array_equal(out["labels"].cpu().numpy(), labels)
        assert np.array_equal(out["table"].numpy(), T._territory_tally_numpy(labels, K, other, 1, region))
    return call, reference


case("territory.partition", ["ru3d_edt_workspace_bytes", "ru3d_skeleton_workspace_bytes"])(lambda: _t_partition("euclidean"))
case("territory.partition_geodesic", ["ru3d_geodesic_workspace_bytes"])(lambda: _t_partition("geodesic"))


# ---- geodesic.py (reference: transform._geodesic_numpy, tests/test_gpu_geodesic.py, equality on dist and labels)
@case("geodesic.grow", ["ru3d_geodesic_workspace_bytes"])
def _g_grow():
    """masked, the face steps, anisotropic: the serpentine inside the first tile takes more rounds than the first batch
    has; the seeds 5 and 4 tie at (8, 9, 48); one seed of label 2 is not allowed"""
    seeds, allowed, _, _ = CI.grow_masked()
    s, a = _up(seeds), _pack(allowed)
    before = s.clone(), a.bits.clone()

    def call():
        dist, labels = geodesic.grow(s, a, CI.SAMPLING, None, CI.QUANTUM)
        assert torch.equal(s, before[0]) and torch.equal(a.bits, before[1])
        return dict(dist=dist.view(torch.int32), labels=labels, rounds=geodesic.last_rounds)

    def reference(out):
        want = CI.grow_twin(seeds, allowed, 1)
        assert int(out["rounds"]) > CI.FLOOD_FIRST_BATCH, "one batch of rounds: %d" % int(out["rounds"])
        assert np.array_equal(out["dist"].cpu().numpy().view(np.uint32), want[0])
        assert np.array_equal(out["labels"].cpu().numpy(), want[1])
    return call, reference


@case("geodesic.grow_cube", ["ru3d_geodesic_workspace_bytes"])
def _g_grow_cube():
    """masked, all 26 steps: four seeds dropped on the speckle mask wherever they fall, one label twice"""
    allowed = _volumes()["mask"]
    seeds = np.zeros(VOL, dtype=np.int32)
    seeds.reshape(-1)[np.random.RandomState(67).choice(seeds.size, 4, replace=False)] = (5, 1, 3, 3)
    s, a = _up(seeds), _pack(allowed)

    def call():
        dist, labels = geodesic.grow(s, a, CI.SAMPLING, CI.CUBE)
        return dict(dist=dist.view(torch.int32), labels=labels, rounds=geodesic.last_rounds)

    def reference(out):
        want = CI.grow_twin(seeds, allowed, 3)
        assert np.array_equal(out["dist"].cpu().numpy().view(np.uint32), want[0])
        assert np.array_equal(out["labels"].cpu().numpy(), want[1])
    return call, reference


@case("geodesic.grow_cube_limit", ["ru3d_geodesic_workspace_bytes"])
def _g_grow_limit():
    """allowed=None (every voxel is allowed, so no seed can lie outside: geodesic.grow has that seed), all 26 steps, a
    max_distance that cuts, every tile in every round"""
    seeds, max_distance = CI.grow_cube()
    s = _up(seeds)

    def call():
        dist, labels = geodesic.grow(s, None, CI.SAMPLING, CI.CUBE, CI.QUANTUM, max_distance, skip_idle=False)
        return dict(dist=dist.view(torch.int32), labels=labels, rounds=geodesic.last_rounds)

    def reference(out):
        want = CI.grow_twin(seeds, None, 3, max_distance)
        dist = out["dist"].cpu().numpy().view(np.uint32)
        assert (dist == geodesic.UNREACHED).any() and np.array_equal(dist, want[0])
        assert np.array_equal(out["labels"].cpu().numpy(), want[1])
    return call, reference


NAMES = list(CASES)
# wrappers that launch an entry point without scratch ahead of their first ask: the sampler its presence kernel (the label
# rule of the patch kernel reads its mask), transform.extract_mesh the pack of the volume, the geodesic partition the
# unpack of the skeleton (the seeds of the growth are the skeleton's voxels, and unpacking needs no scratch)
AHEAD = {"augment.sample": ["augment_label_presence"], "augment.sample_rotation_elastic": ["augment_label_presence"],
         "mesh.extract_measure": ["mask_pack"], "territory.partition_geodesic": ["mask_unpack"]}


# ------------------------------------------------------------------------------------------------ the checks
CALLED = {}             # case -> the entry points of _native.SIGNATURES its first clean run called


@contextlib.contextmanager
def _recorded(into):
    """every entry point of _native.SIGNATURES on N.lib, wrapped as _spied wraps the queries: the names called go `into`"""
    saved = {}
    for n in N.SIGNATURES:
        saved[n] = fn = getattr(N.lib, n)

        def spy(*a, _fn=fn, _n=n):
            into.add(_n)
            return _fn(*a)
        setattr(N.lib, n, spy)
    try:
        yield
    finally:
        for n, fn in saved.items():
            setattr(N.lib, n, fn)


@functools.lru_cache(maxsize=None)
def _clean(name):
    """checks 1 and 2: the clean run, held to the case's reference, then made again: the same launches, the same bits
    (DESIGN's fixed-order reductions - every later comparison stands on it)"""
    call, reference = _built(name)
    with _recorded(CALLED.setdefault(name, set())):        # for the second coverage test; checks 3 to 5 run without it
        names, out, err = _run(call, name)
    assert err is None, err
    print("CLEAN %s %s" % (name, names))
    reference(out)
    names2, out2, err2 = _run(call, name)
    assert err2 is None and names2 == names
    _same(out2, out, "%s: two consecutive clean runs (determinism)" % name)
    return names, out


@pytest.mark.parametrize("name", NAMES)
def test_reference_then_determinism(name):
    _clean(name)


def _bad_label_still_raises(name, byte, what):
    """the out-of-range label of test_gpu_loss_contract.test_a_label_out_of_range, in this file's shape"""
    call, _ = _built(name)
    bad = LOSS_LABELS().clone()
    bad[1, 2, 3, 4] = 3
    L.raise_on_bad_labels(wait=True)
    _, out, err = _run(lambda: call(bad.to(DEV), False), what, alloc=_Alloc(byte))
    assert err is None, err
    with pytest.raises(RuntimeError, match=LC.BAD_LABELS):
        L.raise_on_bad_labels(wait=True)
    assert bool(torch.isnan(out["value"])), "%s: the value of a batch with a bad label is not NaN" % what
    with pytest.raises(RuntimeError, match=LC.BAD_LABELS):
        _run(lambda: call(bad.to(DEV), True), what, alloc=_Alloc(byte))


@pytest.mark.parametrize("name", NAMES)
def test_leftovers_in_scratch_state_and_outputs(name):
    """check 3"""
    names, clean = _clean(name)
    call, _ = _built(name)
    loss = CASES[name][2] == "loss"
    for byte in LEFTOVERS:
        what = "%s with 0x%02X left in the scratch and in what the wrapper allocates" % (name, byte)
        for buf in N._WS.values():
            buf.fill_(byte)
        if loss:
            L.raise_on_bad_labels(wait=True)
        got_names, out, err = _run((lambda: call(None, False)) if loss else call, what, alloc=_Alloc(byte))
        assert err is None, err
        assert got_names == names
        _same(out, clean, what)
        if loss:
            L.raise_on_bad_labels(wait=True)            # in-range labels raise nothing
            for buf in N._WS.values():
                buf.fill_(byte)
            _bad_label_still_raises(name, byte, what)


def _matched(wanted, asks):
    """every wanted size gets an ask of its own, equal or larger, each ask used once: the largest first, each on the
    smallest ask left that holds it -> the sizes left without one"""
    left, missing = sorted(asks), []
    for v in sorted(wanted, reverse=True):
        fit = [a for a in left if a >= v]
        if fit:
            left.remove(fit[0])
        else:
            missing.append(v)
    return missing


@pytest.mark.parametrize("name", NAMES)
def test_scratch_of_exactly_the_asked_size(name):
    """check 4"""
    names, clean = _clean(name)
    call, _ = _built(name)
    queries = CASES[name][1]
    scratch, alloc = _Scratch(), _Alloc(0xFF)
    with _spied(queries) as seen:
        got_names, out, err = _run(call, name, scratch=scratch, alloc=alloc)
    print("SCRATCH %s: asked %s bytes; %s" % (name, scratch.queries, seen))
    assert err is None, err
    assert got_names == names
    _same(out, clean, "%s on a scratch of exactly %s bytes" % (name, scratch.queries))
    assert scratch.guard_intact(), "%s wrote behind the %s bytes it asked for" % (name, scratch.queries)
    for q, values in seen.items():
        assert values, "%s never asked %s" % (name, q)
    kind = CASES[name][2]
    scratch_wanted = [v for q, values in seen.items() if q.endswith("_workspace_bytes") for v in values]
    if kind == "joint_ask":             # degrade.workspace: both layouts, the first rounded up to 256 bytes, in one ask
        scratch_wanted = [sum(scratch_wanted)]
    # the scratch queries against the asks of N.workspace (the renderer: against the uint8 vector it allocates itself),
    # the state queries against the uint8 vectors the wrapper allocates, and against nothing else
    asks = alloc.sizes if kind == "own_scratch" else scratch.queries
    missing = _matched(scratch_wanted, asks)
    assert not missing, "%s: the queries want %s bytes, the asks are %s: nothing holds %s" % (name, scratch_wanted, asks, missing)
    state_wanted = [v for q, values in seen.items() if q.endswith("_state_bytes") for v in values]
    missing = _matched(state_wanted, alloc.sizes)
    assert not missing, "%s: the state queries want %s bytes, the wrapper allocated %s" % (name, state_wanted, alloc.sizes)


@pytest.mark.parametrize("name", NAMES)
def test_scratch_16_bytes_short_is_refused_before_any_launch(name):
    """check 5, for each ask of the call in turn"""
    clean_names, _ = _clean(name)
    call, _ = _built(name)
    probe, probe_alloc = _Scratch(), _Alloc(0xFF)
    with _spied(CASES[name][1]) as seen:
        _run(call, name, scratch=probe, alloc=probe_alloc)
    if CASES[name][2] == "own_scratch":
        # the wrapper's own torch.empty of the queried size comes 16 bytes short
        need = seen["ru3d_render_surface_workspace_bytes"][0]
        alloc = _Alloc(0xFF, shrink={need: SHORT})
        got_names, _, err = _run(call, name, alloc=alloc)
        print("SHORT %s: %s" % (name, err))
        assert err is not None, "%s ran on a scratch %d bytes short of %d" % (name, SHORT, need)
        assert got_names == [], "%s launched %s and then refused its scratch" % (name, got_names)
        assert all(bool((buf[:size] == 0xFF).all()) for buf, size in alloc.made)
        return
    tried = 0
    for k, asked in enumerate(probe.queries):
        if asked < SHORT:
            continue
        tried += 1
        alloc = _Alloc(0xFF)
        short = _Scratch(short=SHORT, only=k, alloc=alloc)
        got_names, _, err = _run(call, name, scratch=short, alloc=alloc)
        what = "%s, ask %d (%d bytes) %d short" % (name, k, asked, SHORT)
        print("SHORT %s: %s" % (what, err))
        assert err is not None, "%s: ran" % what
        assert got_names == [], "%s: launched %s after the ask and then refused" % (what, got_names)
        # and ahead of the ask only what the clean run launches there; ahead of the first ask nothing at all (the
        # launch log of the whole call is empty), but for the wrappers of AHEAD
        assert short.before == clean_names[:len(short.before)], "%s: launched %s ahead of the ask" % (what, short.before)
        if k == 0:
            assert short.before == AHEAD.get(name, []), "%s: launched %s ahead of its first ask" % (what, short.before)
        assert short.guard_intact(), "%s: wrote behind the scratch" % what
        assert alloc.unchanged_since(short.snap), "%s: wrote to what the wrapper had allocated" % what
    if not tried:
        print("SHORT %s: no scratch - nothing to hold" % name)
        assert not probe.queries or max(probe.queries) < SHORT


# ------------------------------------------------------------------------------------------------ coverage
# held by tests/test_gpu_conv_contract.py (EXTRA and the routing tables) and tests/test_gpu_chanloop.py
CONV_AND_NORM = {
    "ru3d_conv3d_workspace_bytes", "ru3d_conv3d_fwd_in_workspace_bytes", "ru3d_conv3d_fwd_in_lrelu_workspace_bytes",
    "ru3d_conv3d_s2_pair_fwd_in_workspace_bytes", "ru3d_conv3d_wgrad_workspace_bytes",
    "ru3d_conv3d_wgrad_bias_workspace_bytes", "ru3d_conv3d_wgrad_pair_workspace_bytes", "ru3d_head_bwd_workspace_bytes",
    "ru3d_convtranspose3d_k3s2p1_fwd_in_workspace_bytes", "ru3d_convtranspose3d_k3s2p1_wgrad_workspace_bytes",
    "ru3d_reduce_workspace_bytes", "ru3d_head_in_bwd_workspace_bytes", "ru3d_conv3d_dgrad_in_bwd_workspace_bytes",
}
TOOL_ONLY = {"ru3d_topk_loss_fwd_timed", "ru3d_topk_loss_fwd_launches"}


def test_every_query_of_the_signature_table_has_a_case():
    wanted = {n for n in N.SIGNATURES if n.endswith("_workspace_bytes") or n.endswith("_state_bytes")}
    assert CONV_AND_NORM <= wanted, "the exclusion list names %s, which the table does not have" % (CONV_AND_NORM - wanted)
    wanted = wanted - CONV_AND_NORM - TOOL_ONLY
    named = {q for _, queries, _ in CASES.values() for q in queries}
    assert named <= wanted, "cases name %s, no query of the table" % sorted(named - wanted)
    assert wanted <= named, "no case for %s" % sorted(wanted - named)


# entry points no case of this table calls, and the file under tests/ that holds each (its text names the entry point): the
# conv, norm and pool families, the optimizers and loss scaling, comm / probe / cu_budget, the predict, cascade and
# render-tile entry points that neither carve nor allocate, the *_supported and layout queries.  The two of TOOL_ONLY
# are called by tools/topk_loss_bench.py alone and named by no test, so no file can stand for them here
HELD_ELSEWHERE = {
    **dict.fromkeys((
        "ru3d_comm_all_gather", "ru3d_comm_allreduce", "ru3d_comm_available", "ru3d_comm_destroy", "ru3d_comm_init",
        "ru3d_comm_reduce_scatter", "ru3d_comm_unique_id", "ru3d_dropout3d_scale", "ru3d_flat_cast",
    ), "tests/dist_child.py"),
    **dict.fromkeys((
        "ru3d_probe_begin", "ru3d_probe_end",
    ), "tests/test_gpu_bench.py"),
    **dict.fromkeys((
        "ru3d_get_cu_budget", "ru3d_set_cu_budget",
    ), "tests/test_gpu_boundary.py"),
    **dict.fromkeys((
        "ru3d_add", "ru3d_affine_lrelu_fwd", "ru3d_batchnorm_bwd_apply", "ru3d_batchnorm_bwd_pool",
        "ru3d_batchnorm_stats_finalize", "ru3d_batchnorm_stats_pool", "ru3d_cast_f32", "ru3d_channel_sum",
        "ru3d_conv3d_dgrad_in_bwd", "ru3d_copy_channels", "ru3d_head_in_bwd", "ru3d_in_lrelu_bwd",
        "ru3d_in_lrelu_bwd_apply", "ru3d_in_lrelu_fwd", "ru3d_instnorm_stats", "ru3d_last_error",
        "ru3d_ncdhw_to_ndhwc", "ru3d_ndhwc_to_ncdhw", "ru3d_pointwise", "ru3d_reduce_workspace_bytes",
    ), "tests/test_gpu_chanloop.py"),
    **dict.fromkeys((
        "ru3d_conv3d_fwd", "ru3d_convtranspose3d_k3s2p1_fwd_in", "ru3d_head_bwd_supported",
        "ru3d_head_bwd_workspace_bytes", "ru3d_head_in_bwd_supported", "ru3d_head_in_bwd_workspace_bytes",
        "ru3d_skip1x1_in_lrelu_fwd_supported",
    ), "tests/test_gpu_conv_contract.py"),
    **dict.fromkeys((
        "ru3d_conv3d_fwd_in_workspace_bytes", "ru3d_conv3d_s2_pair_fwd_in",
        "ru3d_conv3d_s2_pair_fwd_in_workspace_bytes", "ru3d_conv3d_wgrad_pair", "ru3d_conv3d_wgrad_pair_supported",
        "ru3d_conv3d_wgrad_pair_workspace_bytes", "ru3d_conv3d_wgrad_workspace_bytes",
        "ru3d_convtranspose3d_k3s2p1_wgrad_workspace_bytes", "ru3d_set_cu_budget_device",
    ), "tests/test_gpu_cu_budget.py"),
    **dict.fromkeys((
        "ru3d_conv3d_plan_names",
    ), "tests/test_gpu_direct_plan.py"),
    **dict.fromkeys((
        "ru3d_dropout3d_scale_dev",
    ), "tests/test_gpu_graph.py"),
    **dict.fromkeys((
        "ru3d_loss_state_bad_labels_offset", "ru3d_predict_accumulate", "ru3d_predict_accumulate_groups",
        "ru3d_predict_merge", "ru3d_predict_merge_groups",
    ), "tests/test_gpu_groups.py"),
    **dict.fromkeys((
        "ru3d_head_bwd", "ru3d_skip1x1_in_lrelu_fwd", "ru3d_skip1x1_in_lrelu_head_fwd",
        "ru3d_skip1x1_in_lrelu_head_fwd_supported",
    ), "tests/test_gpu_head_tail.py"),
    **dict.fromkeys((
        "ru3d_conv3d_wgrad_bias",
    ), "tests/test_gpu_headstem.py"),
    **dict.fromkeys((
        "ru3d_ds_loss_ignore_bwd", "ru3d_ds_loss_ignore_fwd", "ru3d_loss_ignore_bwd", "ru3d_loss_ignore_fwd",
        "ru3d_topk_loss_ignore_bwd", "ru3d_topk_loss_ignore_fwd",
    ), "tests/test_gpu_ignore_label.py"),
    **dict.fromkeys((
        "ru3d_convtranspose3d_k3s2p1_dgrad", "ru3d_convtranspose3d_k3s2p1_fwd", "ru3d_convtranspose3d_k3s2p1_wgrad",
    ), "tests/test_gpu_inner_boundaries.py"),
    **dict.fromkeys((
        "ru3d_mask_bytes",
    ), "tests/test_gpu_morphology.py"),
    **dict.fromkeys((
        "ru3d_adam_multi", "ru3d_adam_multi_amp", "ru3d_adam_multi_dev", "ru3d_adam_step", "ru3d_amp_update",
        "ru3d_grad_scale_check",
    ), "tests/test_gpu_optim_kernels.py"),
    **dict.fromkeys((
        "ru3d_adam_multi_clip", "ru3d_adam_multi_clip_dev", "ru3d_adamw_multi", "ru3d_adamw_multi_dev",
        "ru3d_grad_norm", "ru3d_grad_norm_finish", "ru3d_grad_scale_dev", "ru3d_grad_sumsq", "ru3d_sgd_multi",
        "ru3d_sgd_multi_dev",
    ), "tests/test_gpu_optim_recipe.py"),
    **dict.fromkeys((
        "ru3d_conv3d_s1_dgrad_pair", "ru3d_conv3d_s2_dgrad_pair",
    ), "tests/test_gpu_pairs.py"),
    **dict.fromkeys((
        "ru3d_conv3d_fwd_in", "ru3d_version",
    ), "tests/test_gpu_parity.py"),
    **dict.fromkeys((
        "ru3d_maxpool3d_bwd", "ru3d_maxpool3d_fwd",
    ), "tests/test_gpu_plain_unet.py"),
    **dict.fromkeys((
        "ru3d_predict_accumulate_weighted", "ru3d_predict_gather",
    ), "tests/test_gpu_predict_tta.py"),
    **dict.fromkeys((
        "ru3d_conv3d_wgrad",
    ), "tests/test_gpu_reduce_tails.py"),
    **dict.fromkeys((
        "ru3d_conv3d_dgrad", "ru3d_pack_weight", "ru3d_pack_weights", "ru3d_packed_weight_bytes",
        "ru3d_unpad_weight_grad",
    ), "tests/test_gpu_round2.py"),
    **dict.fromkeys((
        "ru3d_conv3d_workspace_bytes",
    ), "tests/test_gpu_s1_routing.py"),
    **dict.fromkeys((
        "ru3d_conv3d_fwd_in_lrelu", "ru3d_conv3d_fwd_in_lrelu_workspace_bytes",
    ), "tests/test_gpu_small_norm.py"),
    **dict.fromkeys((
        "ru3d_topk_select_trip_elements",
    ), "tests/test_gpu_topk.py"),
    **dict.fromkeys((
        "ru3d_render_tiles",
    ), "tests/test_gpu_visualize.py"),
    **dict.fromkeys((
        "ru3d_augment_intensity",
    ), "tests/test_host_augment_degrade.py"),
    **dict.fromkeys((
        "ru3d_cascade_merge", "ru3d_region_accumulate",
    ), "tests/test_host_components.py"),
    **dict.fromkeys((
        "ru3d_conv3d_dgrad_in_bwd_workspace_bytes", "ru3d_conv3d_s1_dgrad_pair_supported",
        "ru3d_planar_concat_supported",
    ), "tests/test_host_conv_plan.py"),
    **dict.fromkeys((
        "ru3d_ds_block_bytes", "ru3d_ds_state_bad_labels_offset",
    ), "tests/test_host_deepsup.py"),
    **dict.fromkeys((
        "ru3d_conv3d_s2_dgrad_pair_supported", "ru3d_conv3d_s2_pair_fwd_in_supported",
        "ru3d_convtranspose3d_k3s2p1_fwd_in_workspace_bytes",
    ), "tests/test_host_direct_plan.py"),
    **dict.fromkeys((
        "ru3d_mesh_smooth",
    ), "tests/test_host_mesh.py"),
    **dict.fromkeys((
        "ru3d_conv3d_wgrad_bias_workspace_bytes",
    ), "tests/test_host_wgrad_plan.py"),
}


def test_every_entry_point_of_the_signature_table_is_called_by_a_case_or_held_elsewhere():
    called = set()
    for name in NAMES:
        _clean(name)
        called |= CALLED[name]
    assert called <= set(N.SIGNATURES)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for entry, path in HELD_ELSEWHERE.items():
        assert entry in N.SIGNATURES, "HELD_ELSEWHERE names %s, no entry point of the table" % entry
        assert path.startswith("tests/") and os.path.isfile(os.path.join(root, path)), "%s: no file %s" % (entry, path)
        with open(os.path.join(root, path)) as f:
            assert entry in f.read(), "%s does not name %s" % (path, entry)
    both = sorted(called & set(HELD_ELSEWHERE))
    assert not both, "HELD_ELSEWHERE lists %s, which a case of this table calls" % both
    assert not TOOL_ONLY & (called | set(HELD_ELSEWHERE))
    missing = sorted(set(N.SIGNATURES) - called - set(HELD_ELSEWHERE) - TOOL_ONLY)
    assert not missing, "neither called by a case nor held elsewhere: %s" % missing
