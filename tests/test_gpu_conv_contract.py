"""The conv family's memory and non-finite-value contracts, on the case tables of tests/test_gpu_s1_routing.py and
tests/test_gpu_wgrad_routing.py (their shapes, their expected launch names, asserted first in every run) plus one case
for each entry point (and each fused branch of it) with a *_workspace_bytes query that the tables do not reach, with its
own pinned launch names.  Nothing here needs a reference: every comparison is bit for bit against the same case's own
clean run.  The routing tests hold the same shapes and kernels to float64 on operands of their own seeds; the stride-1
operands here are theirs except that a weight which rounds to zero in the storage type becomes 2^-10 (C needs every
weight non-zero), the weight-gradient operands are drawn here.

  A  scratch      determinism first (two clean runs); then leftovers in every buffer of _native._WS (0x00, 0xFF = NaN,
                  0x7F = 3.4e38) and outputs pre-filled with 0xFF change nothing and leave no NaN; a private scratch of
                  exactly the queried size, filled with NaN, gives the same bits and leaves the 0xA5 guard behind it
                  untouched; 16 bytes fewer are refused before any launch, or (ru3d_conv3d_fwd / _dgrad, whose scratch is
                  optional) run bit for bit what a row of the table runs: the no-scratch kernel (its no_ws rows) or the
                  next kernel of the plan whose partials fit (its short:* rows).
  B  surroundings every 16-bit operand as channels [8, 8 + C) of a NaN-filled buffer 16 channels wider, with a NaN plane
                  before the first sample and after the last; outputs of the library's own allocation as such a slice of
                  a 0xA5-filled buffer: same names, same bits, surroundings of the outputs untouched.
  C  footprint    +-inf / NaN planted in an operand reach exactly the outputs whose receptive field holds them: every such
                  output is non-finite, every other one bit-equal to the clean run.  bf16 and fp16.

The wrappers of _ops are the callers: they hand the C entry points what N.workspace() / N.new_act() and _ops' own
torch.empty() return, so the tests swap those (the last through a stand-in for the name `torch` inside _ops, nowhere
else) for hostile ones around the one call under test and nothing else.
Run with `-m gpu`.  Entry points the wrappers under test go through without the file naming them elsewhere: ops.convt_fwd_in is
ru3d_convtranspose3d_k3s2p1_fwd_in; ops.head_bwd asks ru3d_head_bwd_supported and ru3d_head_bwd_workspace_bytes,
ops.head_in_bwd ru3d_head_in_bwd_supported and ru3d_head_in_bwd_workspace_bytes, ops.skip1x1_in_lrelu_fwd
ru3d_skip1x1_in_lrelu_fwd_supported."""
import contextlib
import functools
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no HIP device", allow_module_level=True)

import _native as N  # noqa: E402
import _ops as ops  # noqa: E402
import test_gpu_s1_routing as S1  # noqa: E402
import test_gpu_wgrad_routing as WG  # noqa: E402

DEV = torch.device("cuda:0")
BF, F16, F32 = torch.bfloat16, torch.float16, torch.float32
NAN, INF = float("nan"), float("inf")
LEFTOVERS = (0x00, 0xFF, 0x7F)
GUARD_MIN = 4 << 20
SLACK = 8           # B: the operand is channels [SLACK, SLACK + C) of a buffer 2 * SLACK channels wider
SHORT = 16

ROUTED = ["s1/" + c for c in sorted(S1.CASES)] + ["wg/" + c for c in sorted(WG.CASES)]
# the entry points with a scratch query that the tables do not reach, at shapes that take the branch which owns scratch:
# the fused forms (slab in the scratch, filled by the conv's epilogue) and, for the dgrad + norm backward, the small-level
# form too (split-K slices in the scratch, summed by the norm kernel).  Shapes of tests/test_gpu_pairs.py, the 64 -> 32
# transposed conv of the decoder, slide32_res's, tests/test_gpu_small_norm.py, test_gpu_headstem.py, test_gpu_head_tail.py
EXTRA_NAMES = {
    "s2_pair_fwd_in": ["conv3_s2_tile", "stats_slab_finalize"],
    "convt_fwd_in": ["convt3_s2_tile", "stats_slab_finalize"],
    "dgrad_in_bwd": ["conv3_s1_slide32<bst>", "bwd_sums_slab_finalize", "in_lrelu_bwd_apply"],
    "dgrad_in_bwd_small": ["conv3_s1_sk<8>", "in_small_bwd"],
    "head_bwd": ["head_bwd", "head_bwd_finalize"],
    "head_in_bwd": ["head_bwd_wgrad", "head_bwd_finalize", "head_in_bwd_reduce", "head_in_bwd_finalize", "head_in_bwd_apply"],
}
EXTRA = ["x/" + c for c in EXTRA_NAMES]


def _names(case):
    kind, cid = case.split("/")
    return S1.CASES[cid][5] if kind == "s1" else WG.CASES[cid][8] if kind == "wg" else EXTRA_NAMES[cid]


def _dtype(case, dt):
    """the fp32 stem case has one storage type"""
    return F32 if case.startswith("wg/") and WG.CASES[case[3:]][1] == F32 else dt


# ------------------------------------------------------------------------------------------------ operands
@functools.lru_cache(maxsize=2)
def _host(case, dt):
    """the case's operands on the host as fp32 values rounded to the storage type; never modified (C clones)"""
    kind, cid = case.split("/")
    if kind == "s1":
        n, cin, cout, dims, what, _ = S1.CASES[cid]
        xv, wt, b, r, gy = S1._operands(n, cin, cout, dims, len(cid) + n + cin + cout + sum(dims))
        # a few of 1.7 M weights of deviation 0.012 fall under fp16's smallest subnormal: C wants every weight non-zero
        wt = torch.where(wt.to(dt) == 0, torch.full_like(wt, 2.0 ** -10), wt)
        return dict(x=xv.to(dt).float(), w=wt, b=b, r=r.to(dt).float(), gy=gy.to(dt).float())
    what, _, n, cin, cout, dims, k, stride, _ = WG.CASES[cid]
    g = torch.Generator().manual_seed(7 + n + cin + cout + sum(dims) + k + stride)
    ydims = tuple(2 * s for s in dims) if what == "convt" else tuple((s - 1) // stride + 1 for s in dims)
    return dict(x=torch.randn((n, cin) + dims, generator=g).to(dt).float(),
                g1=torch.randn((n, cout) + ydims, generator=g).to(dt).float(),
                g2=torch.randn((n, cout) + ydims, generator=g).to(dt).float())


def _slice_of(n, c, d, h, w, dt, fill, lo, wide):
    """channels [lo, lo + c) of a flat buffer `wide` channels wide with one plane (h * w * wide elements) before the first
    sample and one after the last, all of it filled with `fill` (a float, or a byte for an int): (flat, view)"""
    plane, body = h * w * wide, n * d * h * w * wide
    flat = torch.empty(2 * plane + body, dtype=dt, device=DEV)
    if isinstance(fill, int):
        flat.view(torch.uint8).fill_(fill)
    else:
        flat.fill_(fill)
    return flat, flat[plane:plane + body].view(n, d, h, w, wide)[..., lo:lo + c].permute(0, 4, 1, 2, 3)


def _dev(t, dt, poison=False, lo=SLACK, wide=None):
    """t on the device in NDHWC: dense, or (B) as a channel slice of a NaN-filled buffer"""
    n, c, d, h, w = t.shape
    if poison:
        _, v = _slice_of(n, c, d, h, w, dt, NAN, lo, wide or c + 2 * SLACK)
    else:
        v = N.new_act(n, c, d, h, w, dt, DEV)
    v.copy_(t.to(DEV))
    return v


def _prepare(case, dt, h=None, poison=False, arena=False, what_as=None):
    """operands of `case` on the device -> a closure that makes the one call under test and returns its outputs by name.
    h: host operands (default _host); poison: B's surroundings; arena: dW (and dW2) into 0xFF-filled ops.GRAD_ARENA rows"""
    kind, cid = case.split("/")
    if kind == "x":
        return _prepare_extra(cid, dt)
    h = h or _host(case, dt)
    put = lambda t, **kw: _dev(t, dt, poison, **kw)     # noqa: E731
    if kind == "s1":
        n, cin, cout, (d, hh, w), what, _ = S1.CASES[cid]
        what = what_as or what
        if what.startswith("short:"):       # the same call, its scratch 16 bytes under the query
            inner = _prepare(case, dt, h, poison, arena, what_as=what[6:])

            def short():
                with S1.scratch_short_by(SHORT):
                    return inner()
            return short
        if what == "dgrad":
            pw = ops.pack_weight(h["w"].to(DEV), N.ROLE_CONV_DGRAD, dt, 1)
            gyd = put(h["gy"])
            return lambda: dict(dx=ops.conv_dgrad(gyd, pw, (n, cin, d, hh, w), 3, 1))
        pw = ops.pack_weight(h["w"].to(DEV), N.ROLE_CONV_FWD, dt, 1)
        x, bias = put(h["x"]), h["b"].to(DEV)
        if what == "fwd":
            return lambda: dict(y=ops.conv_fwd(x, pw, bias, cout, 3, 1))
        if what == "res":
            res = put(h["r"])
            return lambda: dict(y=ops.conv_fwd(x, pw, bias, cout, 3, 1, res=res))
        if what == "stats":
            return lambda: dict(zip(("y", "mean", "scale"), ops.conv_fwd_in(x, pw, bias, cout, 3, 1)))

        def raw():
            if what == "no_ws":
                y = N.new_act(n, cout, d, hh, w, dt, DEV)
            else:
                y = N.new_act(n, cout + 8, d, hh, w, dt, DEV)[:, 4:4 + cout]
                assert y.data_ptr() % 16 == 8
            N.check(S1._fwd_raw(x, pw, bias, y, with_ws=what != "no_ws"), "conv3d_fwd")
            return dict(y=y)
        return raw
    what, _, n, cin, cout, dims, k, stride, _ = WG.CASES[cid]
    if what == "split":         # the two planes are dense: their surroundings are the planes before and after
        x = N.Split(put(torch.cat((h["x"][:, :cin // 2], h["x"][:, cin // 2:]), dim=0), lo=0, wide=cin // 2))
    elif what == "wide":        # already a slice: the other WIDE - cin channels are the surroundings
        if poison:
            x = put(h["x"], lo=0, wide=WG.WIDE)
        else:
            x = N.new_act(n, WG.WIDE, dims[0], dims[1], dims[2], dt, DEV)[:, :cin]
            x.copy_(h["x"].to(DEV))
    else:
        x = put(h["x"])
    dy = put(h["g1"])
    dy2 = put(h["g2"]) if what == "pair" else None
    wshape = (cin, cout, 3, 3, 3) if what == "convt" else (cout, cin, k, k, k)

    def call():
        keys = {}
        if arena or what == "dw4":
            off = 1 if what == "dw4" else 0
            for key, shape in (("contract", wshape), ("contract2", (cout, cin, 1, 1, 1))):
                numel = 1
                for s in shape:
                    numel *= s
                buf = torch.empty(numel + off, dtype=torch.float32, device=DEV)
                buf.view(torch.uint8).fill_(0xFF)
                ops.GRAD_ARENA[key] = buf[off:].view(shape)
            keys = dict(key="contract")
        try:
            if what == "pair":
                both = ops.conv_wgrad_pair(x, dy, dy2, stride, key2="contract2" if keys else None, **keys)
                assert both is not None, "no pair form for %s" % cid
                out = dict(dw=both[0], dw2=both[1])
            elif what == "bias":
                out = dict(zip(("dw", "db"), ops.conv_wgrad_bias(x, dy, k, stride, **keys)))
            elif what == "convt":
                out = dict(dw=ops.convt_wgrad(x, dy, **keys))
            else:
                out = dict(dw=ops.conv_wgrad(x, dy, k, stride, **keys))
        finally:
            ops.GRAD_ARENA.pop("contract", None)
            ops.GRAD_ARENA.pop("contract2", None)
        if what == "dw4":
            assert out["dw"].data_ptr() % 16 == 4
        return out
    return call


@functools.lru_cache(maxsize=None)
def _extra_operands(cid, dt):
    g = torch.Generator().manual_seed(len(cid))
    rn = lambda *s: torch.randn(*s, generator=g)    # noqa: E731
    if cid == "s2_pair_fwd_in":
        n, cin, cout, (d, h, w) = 2, 32, 64, (16, 40, 80)
        return dict(x=_dev(rn(n, cin, d, h, w), dt), cout=cout,
                    pw3=ops.pack_weight((rn(cout, cin, 3, 3, 3) * (27 * cin) ** -0.5).to(DEV), N.ROLE_CONV_FWD, dt, 2),
                    pw1=ops.pack_weight((rn(cout, cin, 1, 1, 1) * cin ** -0.5).to(DEV), N.ROLE_CONV_FWD, dt, 2),
                    b3=rn(cout).to(DEV), b1=rn(cout).to(DEV))
    if cid == "convt_fwd_in":
        n, cin, cout, (d, h, w) = 2, 64, 32, (16, 32, 32)
        return dict(x=_dev(rn(n, cin, d, h, w), dt), cout=cout, b=rn(cout).to(DEV),
                    pw=ops.pack_weight((rn(cin, cout, 3, 3, 3) * (27 * cin / 8) ** -0.5).to(DEV), N.ROLE_CONVT_FWD, dt))
    if cid in ("dgrad_in_bwd", "dgrad_in_bwd_small"):
        n, c, d, h, w = (2, 32, 16, 64, 64) if cid == "dgrad_in_bwd" else (2, 512, 8, 8, 8)
        y1 = _dev(rn(n, c, d, h, w) * 2 + 0.3, dt)
        mean, scale = ops.in_stats(y1)
        return dict(act=ops.in_lrelu_fwd(y1, mean, scale), mean=mean, scale=scale, dy=_dev(rn(n, c, d, h, w), dt),
                    pw=ops.pack_weight((rn(c, c, 3, 3, 3) * (27 * c) ** -0.5).to(DEV), N.ROLE_CONV_DGRAD, dt, 1))
    if cid == "head_bwd":
        n, cin, cout, (d, h, w) = 2, 32, 3, (16, 24, 40)
        return dict(x=_dev(rn(n, cin, d, h, w), dt), gy=N.to_ndhwc((rn(n, cout, d, h, w) * 1e-2).to(DEV)),
                    wt=(rn(cout, cin, 1, 1, 1) * 0.3).to(DEV))
    assert cid == "head_in_bwd"
    n, cin, cout, hc, (d, h, w) = 2, 64, 32, 3, (32, 32, 32)
    x, y2 = _dev(rn(n, cin, d, h, w), dt), _dev(rn(n, cout, d, h, w) * 2 + 0.5, dt)
    mean, scale = ops.in_stats(y2)
    pws = ops.pack_weight((rn(cout, cin, 1, 1, 1) * cin ** -0.5).to(DEV), N.ROLE_CONV_FWD, dt, 1)
    z = ops.skip1x1_in_lrelu_fwd(x, pws, rn(cout).to(DEV), y2, mean, scale)
    assert z is not None
    return dict(z=z, y2=y2, mean=mean, scale=scale, hw=(rn(hc, cout, 1, 1, 1) * 0.3).to(DEV),
                gy=N.to_ndhwc((rn(n, hc, d, h, w) * 1e-2).to(DEV)))


def _prepare_extra(cid, dt):
    o = _extra_operands(cid, dt)
    torch.cuda.synchronize()

    def call():
        if cid == "s2_pair_fwd_in":
            out = ops.conv_s2_pair_fwd_in(o["x"], o["pw3"], o["b3"], o["pw1"], o["b1"], o["cout"])
            names = ("y3", "mean", "scale", "y1")
        elif cid == "convt_fwd_in":
            out, names = ops.convt_fwd_in(o["x"], o["pw"], o["b"], o["cout"]), ("y", "mean", "scale")
        elif cid in ("dgrad_in_bwd", "dgrad_in_bwd_small"):
            out, names = (ops.conv_dgrad_in_bwd(o["dy"], o["pw"], o["act"], o["mean"], o["scale"]),), ("dy",)
        elif cid == "head_bwd":
            out, names = ops.head_bwd(o["x"], o["gy"], o["wt"], True), ("dx", "dw", "db")
        else:
            out = ops.head_in_bwd(o["z"], o["gy"], o["hw"], True, o["y2"], o["mean"], o["scale"])
            names = ("dy", "gpre", "gsum", "dw", "db")
        assert out is not None, "no fused kernel for %s" % cid
        return dict(zip(names, out))
    return call


# ------------------------------------------------------------------------------------------------ hostile surroundings
class _Scratch:
    """stands in for N.workspace around one call: a private buffer of the queried size less `short` bytes, filled with NaN,
    with a guard of 0xA5 behind it in the same allocation (at least as large, never under 4 MiB)"""

    def __init__(self, short=0):
        self.short, self.queries, self.bufs = short, [], []

    def __call__(self, nbytes, device, slot=0):
        nbytes = int(nbytes)
        size = max(nbytes - self.short, 0)
        buf = torch.empty(size + max(nbytes, GUARD_MIN), dtype=torch.uint8, device=device)
        buf[:size].fill_(0xFF)
        buf[size:].fill_(0xA5)
        self.queries.append(nbytes)
        self.bufs.append((buf, size))
        return buf[:size]

    def guard_intact(self):
        return all(bool((buf[size:] == 0xA5).all()) for buf, size in self.bufs)


class _Outputs:
    """stands in for N.new_act (and, through _TorchOfOps, for the torch.empty of _ops) around one call.  "ff": everything
    the wrapper allocates starts as 0xFF bytes.  "slice": every activation the wrapper allocates is a channel slice of a 0xA5-filled buffer (see _slice_of)"""

    def __init__(self, mode):
        self.mode, self.made = mode, []
        self.empty = torch.empty

    def new_act(self, n, c, d, h, w, dtype, device, zero=False):
        assert not zero
        if self.mode == "slice" and dtype != F32:
            flat, v = _slice_of(n, c, d, h, w, dtype, 0xA5, SLACK, c + 2 * SLACK)
            self.made.append((flat, v))
            return v
        return self.filled((n, d, h, w, c), dtype=dtype, device=device).permute(0, 4, 1, 2, 3)

    def filled(self, *a, **kw):
        t = self.empty(*a, **kw)
        if t.numel():
            t.reshape(-1).view(torch.uint8).fill_(0xFF)
        return t

    def surroundings_intact(self):
        """every byte outside the slices is still 0xA5: blank the slices, look at the rest"""
        for flat, v in self.made:
            v.view(torch.int16).fill_(0xA5A5 - 0x10000)
            if not bool((flat.view(torch.uint8) == 0xA5).all()):
                return False
        return True


class _TorchOfOps:
    """what the name `torch` means inside _ops for the length of one call: torch, but for empty()"""

    def __init__(self, empty):
        self.empty = empty

    def __getattr__(self, name):
        return getattr(torch, name)


@contextlib.contextmanager
def _swapped(scratch=None, outputs=None):
    saved = N.workspace, N.new_act, ops.torch
    try:
        if scratch is not None:
            N.workspace = scratch
        if outputs is not None:
            N.new_act = outputs.new_act
            if outputs.mode == "ff":
                ops.torch = _TorchOfOps(outputs.filled)
        yield
    finally:
        N.workspace, N.new_act, ops.torch = saved


def _run(call, scratch=None, outputs=None):
    """the one call inside the launch log -> (names, outputs, error message or None); outputs copied off the arena"""
    err, out = None, {}
    with _swapped(scratch, outputs):
        with ops.launch_log() as log:
            try:
                out = call()
            except N.Ru3dError as e:
                err = str(e)
    torch.cuda.synchronize()
    return log.names, out, err


def _same(a, b, what):
    assert a.keys() == b.keys(), what
    for k in a:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, (what, k)
        same = torch.equal(a[k], b[k])
        assert same, "%s: %s differs in %d of %d elements" % (what, k, int((a[k] != b[k]).sum()), a[k].numel())


def _no_nan(out, what):
    for k, t in out.items():
        assert not bool(torch.isnan(t).any()), "%s: NaN left in %s" % (what, k)


@functools.lru_cache(maxsize=None)
def _clean(case, dt):
    """the case's clean run, made twice: the launch log is the table's and the two runs agree bit for bit (DESIGN's
    fixed-order reductions - every comparison in this file stands on it, so a failure here is a determinism failure)"""
    call = _prepare(case, dt)
    names, out, err = _run(call)
    assert err is None, err
    want = _names(case)
    print("CLEAN %s %s %s" % (case, dt, names))
    assert names == want, "%s ran %s, the table says %s" % (case, names, want)
    names2, out2, err2 = _run(call)
    assert err2 is None and names2 == names
    _same(out2, out, "%s: two consecutive clean runs (determinism)" % case)
    return names, {k: v.clone() for k, v in out.items()}


# ------------------------------------------------------------------------------------------------ A. scratch
def _query(case, dt):
    """what the case's *_workspace_bytes query returns: asked through the wrapper, by a run on a private scratch"""
    s = _Scratch()
    names, out, err = _run(_prepare(case, dt), scratch=s)
    return s, names, out, err


@functools.lru_cache(maxsize=None)
def _has_scratch(case):
    dt = _dtype(case, BF)
    names, _ = _clean(case, dt)
    s = _query(case, dt)[0]
    return len(names) > 1 or any(q > 0 for q in s.queries)


def _ids(cases):
    return [c.split("/")[1] for c in cases]


@pytest.mark.parametrize("case", ROUTED + EXTRA, ids=_ids(ROUTED + EXTRA))
def test_determinism_then_scratch_leftovers(case):
    """A.4 then A.1.  Every case of the tables runs here (a case without scratch must not mind the leftovers either)"""
    dt = _dtype(case, BF)
    names, clean = _clean(case, dt)
    call = _prepare(case, dt, arena=True)
    for byte in LEFTOVERS:
        for buf in N._WS.values():
            buf.fill_(byte)
        got_names, out, err = _run(call, outputs=_Outputs("ff"))
        assert err is None, err
        assert got_names == names
        _same(out, clean, "%s with 0x%02X left in the scratch and 0xFF in the outputs" % (case, byte))
        _no_nan(out, "%s, 0x%02X" % (case, byte))


@pytest.mark.parametrize("case", ROUTED + EXTRA, ids=_ids(ROUTED + EXTRA))
def test_scratch_of_exactly_the_queried_size(case):
    """A.2, and A.3 with 16 bytes fewer"""
    dt = _dtype(case, BF)
    names, clean = _clean(case, dt)
    if not _has_scratch(case):
        print("SCRATCH %s: query 0 and one launch - nothing to hold" % case)
        return
    s, got_names, out, err = _query(case, dt)
    print("SCRATCH %s: queried %s bytes" % (case, s.queries))
    assert err is None, err
    assert got_names == names
    _same(out, clean, "%s on a scratch of exactly %s bytes" % (case, s.queries))
    assert s.guard_intact(), "%s wrote behind the %s bytes it asked for" % (case, s.queries)
    if not any(q >= SHORT for q in s.queries):
        return
    short = _Scratch(short=SHORT)
    got_names, out, err = _run(_prepare(case, dt), scratch=short)
    assert short.guard_intact(), "%s wrote behind a scratch %d bytes short" % (case, SHORT)
    if err is not None:
        print("SHORT %s: refused: %s" % (case, err))
        assert got_names == [], "%s launched %s and then refused its scratch" % (case, got_names)
        return
    # accepted: only the optional scratch of ru3d_conv3d_fwd / _dgrad may be.  The plan is a ladder of kernels and the launch
    # takes the first whose partials fit the scratch it was given.  The last rung needs none: the table's no_ws rows, and
    # the run without scratch must come out bit for bit.  A rung in between (the deepest level: conv_ws wants 8 slices,
    # conv3_s1_sk 4) has a table row of its own, "short:<form>" at this shape: that row's call on these operands, bit for bit
    kind, cid = case.split("/")
    what = S1.CASES[cid][4] if kind == "s1" else None
    print("SHORT %s: ran %s" % (case, got_names))
    if what is not None and what.startswith("short:"):      # such a row itself: its scratch was short all along
        assert got_names == names
        _same(out, clean, "%s: the short row once more" % case)
        return
    assert what in ("fwd", "res", "dgrad"), "%s ran %s on a short scratch" % (case, got_names)
    with_none = ops._conv_ws
    try:
        ops._conv_ws = lambda *a: (None, 0)
        ref_names, ref, err = _run(_prepare(case, dt))
    finally:
        ops._conv_ws = with_none
    assert err is None, err
    if got_names == ref_names:
        assert any(got_names == c[5] and c[4] == "no_ws" for c in S1.CASES.values()), "not a no_ws row of the table"
        _same(out, ref, "%s on a short scratch against the run without scratch" % case)
        return
    rows = [c for c, v in S1.CASES.items() if v[:4] == S1.CASES[cid][:4] and v[4] == "short:" + what]
    assert rows, "%s ran %s on a short scratch: neither the run without scratch (%s) nor a row of the table" % (
        case, got_names, ref_names)
    assert got_names == S1.CASES[rows[0]][5]
    ref_names, ref, err = _run(_prepare("s1/" + rows[0], dt, h=_host(case, dt)))
    assert err is None and ref_names == got_names
    _same(out, ref, "%s on a short scratch against the table's %s" % (case, rows[0]))


# ------------------------------------------------------------------------------------------------ B. surroundings
SLICED = [c for c in ROUTED if not (c.startswith("s1/") and S1.CASES[c[3:]][4] == "y8")]


@pytest.mark.parametrize("case", SLICED, ids=_ids(SLICED))
def test_poisoned_surroundings(case):
    dt = _dtype(case, BF)
    names, clean = _clean(case, dt)
    outs = _Outputs("slice")
    got_names, out, err = _run(_prepare(case, dt, poison=True), outputs=outs)
    assert err is None, err
    assert got_names == names, "%s ran %s on channel slices, %s dense" % (case, got_names, names)
    _same({k: v.contiguous() for k, v in out.items()}, {k: v.contiguous() for k, v in clean.items()},
          "%s with NaN around every operand" % case)
    print("SURROUNDINGS %s: %d pitched outputs" % (case, len(outs.made)))
    assert outs.surroundings_intact(), "%s wrote outside its output's channel slice" % case


# ------------------------------------------------------------------------------------------------ C. footprint
def _nonfinite(t):
    return ~torch.isfinite(t.float())


def _plant(t, ch, spots):
    """spots: (sample, d, h, w, value) -> the planted copy and the [N, D, H, W] mask of voxels within Chebyshev distance 1"""
    t = t.clone()
    n, _, d, h, w = t.shape
    mask = torch.zeros(n, d, h, w, dtype=torch.bool)
    for s, z, y, x, v in spots:
        t[s, ch, z, y, x] = v
        mask[s, max(z - 1, 0):z + 2, max(y - 1, 0):y + 2, max(x - 1, 0):x + 2] = True
    return t, mask


def _spots(n, dims, edge):
    d, h, w = dims
    seam = 32 if w > 32 else w // 2
    last = (n - 1, d // 2, h // 2, w - 1) if edge else (n - 1, 1, h // 2, 1)
    return [(0, 0, 0, 0, INF), (n - 1, d - 1, h - 1, w - 1, -INF), (0, d // 2, h // 2, seam, NAN), last + (INF,)]


FOOT_S1 = [("s1/" + c, dt) for c in sorted(S1.CASES) for dt in (BF, F16)]
FOOT_WG = [("wg/" + c, dt, v) for c in sorted(WG.CASES) for dt in ((BF, F16) if WG.CASES[c][1] == BF else (F32,))
           for v in ("dense_inside", "dense_corner", "gathered_inside")]
_DT = {BF: "bf16", F16: "fp16", F32: "fp32"}


@pytest.mark.parametrize("case,dt", FOOT_S1, ids=["%s-%s" % (c[3:], _DT[t]) for c, t in FOOT_S1])
def test_nonfinite_footprint_forward_and_dgrad(case, dt):
    """The four spots lie in sample 0 and in the last sample, so with the table's n = 1 and n = 2 every sample of a `stats`
    case is planted and the loop over unplanted samples' mean and scale at the end has nothing to run on: it is there for
    a `stats` row with three samples or more.  Planted samples' statistics are not asserted (all their channels are hit)."""
    n, cin, cout, dims, what, names = S1.CASES[case[3:]]
    what = what[6:] if what.startswith("short:") else what
    h = dict(_host(case, dt))
    wr = h["w"].to(dt)
    assert bool((wr != 0).all()), "a weight rounds to zero"
    op, c = ("gy", cout) if what == "dgrad" else ("x", cin)
    h[op], mask = _plant(h[op], c // 2, _spots(n, dims, "edge" in case))
    _, clean = _clean(case, dt)
    got_names, out, err = _run(_prepare(case, dt, h=h))
    assert err is None, err
    assert got_names == names
    y = out["dx" if what == "dgrad" else "y"]
    mask = mask.to(DEV)[:, None].expand_as(y)
    bad = _nonfinite(y)
    print("FOOTPRINT %s %s: %d voxels expected, %d elements non-finite" % (case, _DT[dt], int(mask[:, 0].sum()), int(bad.sum())))
    assert bool(bad[mask].all()), "%s lost a non-finite value at %d elements" % (case, int((~bad & mask).sum()))
    assert torch.equal(y[~mask], clean["dx" if what == "dgrad" else "y"][~mask]), \
        "%s spread a non-finite value to %d elements outside the receptive field" % (case, int((bad & ~mask).sum()))
    if what == "stats":     # every channel of a planted sample is non-finite; the other samples are untouched
        free = (~mask[:, 0].reshape(n, -1).any(dim=1)).nonzero().flatten().tolist()
        for k in ("mean", "scale"):
            for s in free:
                assert torch.equal(out[k].view(n, cout)[s], clean[k].view(n, cout)[s]), (k, s)


def _taps(v, size_g, size_d, k, stride, from_dense):
    """per axis: the taps t with gathered index g = stride * p + t - k // 2 in bounds, given p = v (from_dense) or g = v"""
    if from_dense:
        return [t for t in range(k) if 0 <= stride * v + t - k // 2 < size_g]
    return [t for t in range(k) if (v + k // 2 - t) % stride == 0 and 0 <= (v + k // 2 - t) // stride < size_d]


@pytest.mark.parametrize("case,dt,variant", FOOT_WG, ids=["%s-%s-%s" % (c[3:], _DT[t], v) for c, t, v in FOOT_WG])
def test_nonfinite_footprint_weight_gradient(case, dt, variant):
    """dW[a][b][tap] = sum dense[n, a, p] * gathered[n, b, stride * p + tap - k // 2]: (dense, gathered) = (dy, x) for a
    Conv3d, (x, dy) for the ConvTranspose3d.  An inf in channel a* of dense makes row a* non-finite at every tap whose
    gathered voxel is in bounds (a tap in the padding multiplies inf by an implicit zero: either outcome is allowed) and
    leaves every other row bit-equal; an inf in channel b* of gathered makes dW[:, b*, tap] non-finite at every tap
    through which an output position reads that voxel (with stride 2 that is one tap in two per axis) and leaves the
    other taps of b* and every other b bit-equal.  The pair form is run twice, the inf in dy alone (dW2 bit-equal
    throughout) and in dy2 alone (dW bit-equal throughout), so a leak from one gradient into the other shows."""
    what, _, n, cin, cout, dims, k, stride, names = WG.CASES[case[3:]]
    h = dict(_host(case, dt))
    dn, gn = ("x", "g1") if what == "convt" else ("g1", "x")
    if what == "convt":
        k, stride = 3, 2
    dense, gath = h[dn], h[gn]
    sd, sg = dense.shape[2:], gath.shape[2:]
    if variant == "gathered_inside":
        v = [(s // 2) // stride * stride for s in sg]
        ch = gath.shape[1] // 2
        taps = [_taps(v[a], sg[a], sd[a], k, stride, False) for a in range(3)]
        for t in itertools.product(*taps):      # the dense values that meet the planted one are not zero
            p = [(v[a] + k // 2 - t[a]) // stride for a in range(3)]
            assert bool((dense[0, :, p[0], p[1], p[2]] != 0).all())
        h[gn] = gath.clone()
        h[gn][0, ch, v[0], v[1], v[2]] = INF
    else:
        v = [0, 0, 0] if variant == "dense_corner" else [min(s // 2, max((sg[a] - 2) // stride, 0)) for a, s in enumerate(sd)]
        ch = dense.shape[1] // 2
        taps = [_taps(v[a], sg[a], sd[a], k, stride, True) for a in range(3)]
        if variant == "dense_inside" and min(sd) > 2:
            assert all(len(t) == k for t in taps), "not an interior voxel"
        for t in itertools.product(*taps):
            q = [stride * v[a] + t[a] - k // 2 for a in range(3)]
            assert bool((gath[0, :, q[0], q[1], q[2]] != 0).all())
        h[dn] = dense.clone()
        h[dn][0, ch, v[0], v[1], v[2]] = INF
        if what == "pair":      # the second run: the inf in dy2 alone
            h2 = dict(_host(case, dt))
            h2["g2"] = h2["g2"].clone()
            h2["g2"][0, ch, v[0], v[1], v[2]] = INF
    _, clean = _clean(case, dt)
    got_names, out, err = _run(_prepare(case, dt, h=h))
    assert err is None, err
    assert got_names == names
    dw, ref = out["dw"], clean["dw"]
    hit = torch.zeros(k, k, k, dtype=torch.bool)
    for t in itertools.product(*taps):
        hit[t] = True
    hit = hit.to(DEV)
    axis = 1 if variant == "gathered_inside" else 0
    others = [i for i in range(dw.shape[axis]) if i != ch]
    sel = dw.select(axis, ch)
    print("FOOTPRINT %s %s %s: %d of %d taps reached" % (case, _DT[dt], variant, int(hit.sum()), k ** 3))
    assert bool(_nonfinite(sel)[..., hit].all()), "%s lost the inf at %d entries" % (
        case, int((~_nonfinite(sel)[..., hit]).sum()))
    idx = torch.tensor(others, device=DEV)
    assert torch.equal(dw.index_select(axis, idx), ref.index_select(axis, idx)), "%s spread the inf to other channels" % case
    if variant == "gathered_inside":    # no output position reads the planted voxel through the other taps
        assert torch.equal(sel[..., ~hit], ref.select(axis, ch)[..., ~hit]), "%s spread the inf to %d taps that never read it" % (
            case, int(_nonfinite(sel)[..., ~hit].sum()))
    if "dw2" in out and variant == "gathered_inside":       # the 1x1x1 conv of the same stride reads x[stride * p]
        assert all(c % stride == 0 for c in v)
        assert bool(_nonfinite(out["dw2"].select(axis, ch)).all()), "dW2 lost the inf"
        assert torch.equal(out["dw2"].index_select(axis, idx), clean["dw2"].index_select(axis, idx))
    elif "dw2" in out:
        assert torch.equal(out["dw2"], clean["dw2"]), "the inf in dy reached dW2"
        got_names, out2, err = _run(_prepare(case, dt, h=h2))
        assert err is None and got_names == names
        assert torch.equal(out2["dw"], ref), "the inf in dy2 reached dW"
        assert bool(_nonfinite(out2["dw2"].select(0, ch)).all()), "dW2 lost the inf"
        assert torch.equal(out2["dw2"].index_select(0, idx), clean["dw2"].index_select(0, idx))
    if "db" in out:
        if variant == "gathered_inside":
            assert torch.equal(out["db"], clean["db"])
        else:
            assert not bool(torch.isfinite(out["db"][ch])), "db lost the inf"
            keep = torch.tensor(others, device=DEV)
            assert torch.equal(out["db"][keep], clean["db"][keep])
