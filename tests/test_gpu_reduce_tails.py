"""The second stages of the fixed-order reductions and the cross-lane tails of their first stages, at the row counts where
a hoisted or batched load can go wrong: one row, and one below, at and above each batch size and the lane count.

The contract under test (csrc/norm.hip, above FIN_CX): the value an output receives is one fixed sequence of
floating-point operations on fixed operands; only when the loads are issued and which thread runs a chain is free.  So:

  norm finalizes    stats_finalize / bwd_finalize / chansum_finalize read partials that live in the CALLER's workspace
                    (part[((n * chunks + chunk) * C + c) * 2 + {0, 1}] as doubles, m12 right behind them, the apply
                    pass's dy-sum partials behind that).  The test reads the partials back and redoes the second stage
                    on the host in float64 in the documented order (lane ky = rows ky, ky + 16, ... ascending; then the
                    16 lanes in order).  mean, m12, gpre_sum and dy_sum are a sum times a constant rounded once: bit for
                    bit.  scale has a square root and a division in between: one float ulp.
  slab finalize     the sliding conv's statistics against ru3d_instnorm_stats on the stored output, at the tolerance
                    tests/test_gpu_pairs.py uses for that pair.  Equality is not expected: the conv sums its fp32
                    accumulators BEFORE they are rounded to the storage type, the separate pass sums the rounded values.
  slab sums         ru3d_conv3d_wgrad on the integer lattice of tests/test_gpu_inner_boundaries.py (x, dy uniform in
                    {-2 .. 2}: fp32 sums are exact in any order), torch.equal against float64, at slab counts around the
                    batch sizes of each of wgrad_reduce<64>, wgrad_reduce<8> and wgrad_reduce_tiled<true>.  A dropped or
                    repeated slab cannot pass; a reordered one can - bench.py --dump-outputs against the parent is the
                    check for that.
  head finalize     head_bwd_finalize_kernel from the rows head_bwd_kernel left in the scratch, redone on the host in its
                    order (lane l = rows l, l + 64, ...; then wave_sum_d's butterfly): dW and db bit for bit.
  reduce2 tails     the partials themselves against float64 sums over each chunk's voxels, and bit-identical between two
                    calls.

Both 16-bit builds.  Run with `-m gpu`."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no HIP device", allow_module_level=True)

import _native as N  # noqa: E402
import _ops as ops  # noqa: E402
from test_gpu_chanloop import Slab, _in_bwd, _not_small, _vec  # noqa: E402
from test_gpu_inner_boundaries import _lattice, _logged, _wgrad_ref  # noqa: E402
from test_host_norm_ws import chanloop as _chanloop  # noqa: E402

DEV = torch.device("cuda:0")
DTYPES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "fp16"]
IN_EPS = 1e-5
FIN_KY = 16
# Chunk counts = rows of a sample.  A lane of the 16 takes rows ky, ky + 16, ...; a whole batch is FIN_BATCH = 32 rows per lane
# = 512 rows, what is left goes in one guarded batch of 32, or of 8 where no lane has more than eight rows left.
#   1; 15 / 16 / 17: below, at and above the lane count; 31 / 33: two rows on some lanes
#   128 / 129: eight rows per lane (the short guarded batch) and nine on lane 0 (the long one)
#   255 / 256 / 257: sixteen rows per lane, half a batch
#   511 / 512 / 513: one row short of a whole batch (guarded, lane 15 short), exactly one whole batch and nothing left,
#                    one whole batch and a single row left on lane 0
#   640 / 641: a whole batch, then eight rows per lane / nine on lane 0: the choice between the guarded batches after a
#              whole one
#   1000, 1041, 1200: one or two whole batches and a ragged rest (1024 - the benchmark's level 0 - has none)
# make_chanloop aims at 2048 workgroups, so a sample of a batch of n has at most 2048 / n chunks: _chunks(n) drops the rest.
CHUNKS = [1, 15, 16, 17, 31, 33, 128, 129, 255, 256, 257, 511, 512, 513, 640, 641, 1000, 1041, 1200]


def _chunks(n):
    return [k for k in CHUNKS if k * n <= 2048]


def _values(n, c, V, g):
    """normal data, one channel with a mean 50 times the spread: a dropped or doubled row moves its sums by far more
    than an ulp"""
    y = torch.randn(n, c, 1, 1, V, generator=g) * 1.5 + 0.2
    y[:, 3] += 75.0
    return y


def _ws(nbytes):
    buf = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 256 == 0
    return buf


def _doubles(ws, offset, count):
    return ws[offset:offset + 8 * count].cpu().numpy().view(np.float64).copy()


def _floats(ws, offset, count):
    return ws[offset:offset + 4 * count].cpu().numpy().view(np.float32).copy()


def _finalize64(rows):
    """finalize_sums on the host: rows [R][C][2] float64 -> [C][2]; lane ky adds rows ky, ky + 16, ... ascending, then the
    lanes are added in lane order, all from 0.0"""
    lanes = np.zeros((FIN_KY,) + rows.shape[1:], dtype=np.float64)
    for r in range(rows.shape[0]):
        lanes[r % FIN_KY] += rows[r]
    t = np.zeros(rows.shape[1:], dtype=np.float64)
    for k in range(FIN_KY):
        t += lanes[k]
    return t


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _stats_case(dt, n, c, V, vec):
    """ru3d_instnorm_stats on a dense [n][V][c] tensor -> (y slab, part [n][chunks][c][2], mean, scale)"""
    g = torch.Generator().manual_seed(n * 1000 + c + V)
    y = Slab(n, c, (1, 1, V), None, dt, _values(n, c, V, g))
    assert _vec(dt, c, y) == vec
    chunks = _chanloop(V, c, vec, 64, n)[4]
    dyy = y.desc()
    nbytes = N.lib.ru3d_reduce_workspace_bytes(N.ref(dyy))
    ws = _ws(nbytes)
    mean = torch.empty(n * c, dtype=torch.float32, device=DEV)
    scale = torch.empty(n * c, dtype=torch.float32, device=DEV)
    N.check(N.lib.ru3d_instnorm_stats(N.ref(dyy), None, N.ptr(mean), N.ptr(scale), ctypes.c_void_p(ws.data_ptr()), nbytes,
                                      IN_EPS, N.dtype_code(dt), N.stream(DEV)), "instnorm_stats")
    torch.cuda.synchronize()
    part = _doubles(ws, 0, n * chunks * c * 2).reshape(n, chunks, c, 2)
    return y, part, mean.cpu().numpy(), scale.cpu().numpy()


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", [1, 2, 3])
def test_stats_finalize_order(n, dt):
    """stats_finalize_kernel: mean bit for bit, scale within one ulp of the float64 second stage on the kernel's own
    partials.  C = 32 at width 8 gives spans of 256 voxels; one ragged V, and C = 64 once."""
    cases = [(32, 256 * k, k) for k in _chunks(n)] + [(32, 256 * 17 + 5, 18), (32, 256 * 512 + 5, 513), (64, 128 * 33, 33)]
    for c, V, want_chunks in cases:
        span, chunks = _chanloop(V, c, 8, 64, n)[3:]
        assert (span, chunks) == (256 if c == 32 else 128, want_chunks), (c, V, span, chunks)
        _, part, mean, scale = _stats_case(dt, n, c, V, 8)
        inv = 1.0 / float(V)
        eps = float(np.float32(IN_EPS))
        for i in range(n):
            t = _finalize64(part[i])
            m = t[:, 0] * inv
            var = np.maximum(t[:, 1] * inv - m * m, 0.0)
            what = "n=%d/%d C=%d V=%d chunks=%d" % (i, n, c, V, chunks)
            assert np.array_equal(_bits(mean[i * c:(i + 1) * c]), _bits(m.astype(np.float32))), "mean " + what
            ref = (1.0 / np.sqrt(var + eps)).astype(np.float32)
            err = np.abs(scale[i * c:(i + 1) * c].astype(np.float64) - ref.astype(np.float64))
            assert bool((err <= np.spacing(ref).astype(np.float64)).all()), "scale %s: %g" % (what, err.max())


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", [1, 2, 3])
def test_bwd_finalize_order(n, dt):
    """bwd_finalize_kernel (m12 and gpre_sum) and chansum_finalize_kernel (dy_sum, N * chunks' rows: up to 3 x 641 and
    2 x 1000) through ru3d_in_lrelu_bwd's residual form.  The operands sit at pitch 36, offset 4: width 4 (spans
    of 128 voxels) and no whole-instance kernel of norm_small.hip, which has no partials."""
    c, lay = 32, (36, 4)
    for V, k in [(128 * k, k) for k in _chunks(n)] + [(128 * 17 + 5, 18)]:
        dims = (1, 1, V)
        g = torch.Generator().manual_seed(n * 100 + V)
        y = Slab(n, c, dims, lay, dt, _values(n, c, V, g))
        gout = Slab(n, c, dims, lay, dt, torch.randn((n, c) + dims, generator=g) + 0.3)
        res = Slab(n, c, dims, lay, dt, torch.randn((n, c) + dims, generator=g) * 0.5)
        out, dy, gpre = (Slab(n, c, dims, lay, dt) for _ in range(3))
        assert _vec(dt, c, y, gout, out, dy, gpre) == 4 and _not_small(dt, c, dims, y, gout, out, dy, gpre)
        span, chunks = _chanloop(V, c, 4, 64, n)[3:]
        chunks_a = _chanloop(V, c, 4, 16, n)[4]
        assert (span, chunks) == (128, k), (V, span, chunks)
        mean, scale = ops.in_stats(y.t)
        ops.in_lrelu_fwd(y.t, mean, scale, res=res.t, out=out.t)
        nbytes = N.lib.ru3d_reduce_workspace_bytes(N.ref(y.desc()))
        ws = _ws(nbytes)
        gsum = torch.full((c,), float("nan"), dtype=torch.float32, device=DEV)
        dsum = torch.full((c,), float("nan"), dtype=torch.float32, device=DEV)
        N.check(_in_bwd(gout, out, y, mean, scale, dy, gpre, False, gsum, dsum, ctypes.c_void_p(ws.data_ptr()), nbytes),
                "in_lrelu_bwd")
        torch.cuda.synchronize()
        off_m12 = n * chunks * c * 16
        off_dpart = off_m12 + -(-(n * c * 8) // 256) * 256
        part = _doubles(ws, 0, n * chunks * c * 2).reshape(n, chunks, c, 2)
        m12 = _floats(ws, off_m12, n * c * 2).reshape(n, c, 2)
        dpart = _doubles(ws, off_dpart, n * chunks_a * c * 2).reshape(n * chunks_a, c, 2)
        inv = 1.0 / float(V)
        s = np.zeros(c, dtype=np.float64)
        what = "N=%d V=%d chunks=%d" % (n, V, chunks)
        for i in range(n):
            want = (_finalize64(part[i]) * inv).astype(np.float32)
            assert np.array_equal(_bits(m12[i]), _bits(want)), "m12 of sample %d, %s" % (i, what)
            s += want[:, 0].astype(np.float64)
        assert np.array_equal(_bits(gsum.cpu().numpy()), _bits((s * float(V)).astype(np.float32))), "gpre_sum " + what
        want = _finalize64(dpart)[:, 0].astype(np.float32)
        assert np.array_equal(_bits(dsum.cpu().numpy()), _bits(want)), "dy_sum " + what
        assert bool((dpart[:, :, 1] == 0.0).all())


# (C, V, n, width): 64 channels (Gb = 8, vpb = 32); G = 3 (vpb = 85, thread 255 idle); two group blocks, the second with
# one live group of 256 (G = 257: the chains of a block outnumber its threads); the level-0 shape of the bullets above
TAIL_CASES = [(64, 128 * 3 + 7, 2, 8), (24, 1000, 2, 8), (2056, 37, 2, 8), (32, 256 * 2 + 5, 1, 8)]


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("c,V,n,vec", TAIL_CASES, ids=["c64", "g3", "g257", "c32"])
def test_reduce2_tail_partials(c, V, n, vec, dt):
    """reduce2_kernel's partials: every (sample, chunk, channel) pair against the float64 sums over the chunk's voxels
    of the stored tensor, at the bound tests/test_gpu_chanloop.py holds channel sums to (2e-6 of the sum of magnitudes
    + 1e-6), and the same bits from a second call."""
    y, part, _, _ = _stats_case(dt, n, c, V, vec)
    _, part2, _, _ = _stats_case(dt, n, c, V, vec)
    assert np.array_equal(part.view(np.int64), part2.view(np.int64)), "partials differ between two calls"
    span, chunks = _chanloop(V, c, vec, 64, n)[3:]
    yd = y.f64().reshape(n, c, V).numpy()
    for k in range(chunks):
        seg = yd[:, :, k * span:min(V, (k + 1) * span)]
        for j, (ref, mag) in enumerate(((seg.sum(axis=2), np.abs(seg).sum(axis=2)), ((seg * seg).sum(axis=2),) * 2)):
            err = np.abs(part[:, k, :, j] - ref)
            assert bool((err <= 2e-6 * mag + 1e-6).all()), "sum %d of chunk %d: %g" % (j, k, err.max())


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_dysum_tail_partials(dt):
    """in_lrelu_bwd_kernel's dy-sum epilogue (one chain per channel): the partials against float64 sums of the stored dy,
    same bound; C = 64 at width 8 (V > 8192 keeps norm_small.hip out)."""
    n, c, dims = 2, 64, (1, 3, 2741)
    V = dims[1] * dims[2]
    g = torch.Generator().manual_seed(64)
    y = Slab(n, c, dims, None, dt, _values(n, c, V, g).reshape((n, c) + dims))
    gout = Slab(n, c, dims, None, dt, torch.randn((n, c) + dims, generator=g) + 0.3)
    out, dy = Slab(n, c, dims, None, dt), Slab(n, c, dims, None, dt)
    assert _vec(dt, c, y, gout, out, dy) == 8 and _not_small(dt, c, dims, y, gout, out, dy)
    mean, scale = ops.in_stats(y.t)
    ops.in_lrelu_fwd(y.t, mean, scale, out=out.t)
    nbytes = N.lib.ru3d_reduce_workspace_bytes(N.ref(y.desc()))
    ws = _ws(nbytes)
    dsum = torch.full((c,), float("nan"), dtype=torch.float32, device=DEV)
    N.check(_in_bwd(gout, out, out, mean, scale, dy, None, False, None, dsum, ctypes.c_void_p(ws.data_ptr()), nbytes),
            "in_lrelu_bwd")
    torch.cuda.synchronize()
    chunks = _chanloop(V, c, 8, 64, n)[4]
    span_a, chunks_a = _chanloop(V, c, 8, 16, n)[3:]
    off = n * chunks * c * 16 + -(-(n * c * 8) // 256) * 256
    dpart = _doubles(ws, off, n * chunks_a * c * 2).reshape(n, chunks_a, c, 2)
    st = dy.f64().reshape(n, c, V).numpy()
    for k in range(chunks_a):
        seg = st[:, :, k * span_a:min(V, (k + 1) * span_a)]
        err = np.abs(dpart[:, k, :, 0] - seg.sum(axis=2))
        assert bool((err <= 2e-6 * np.abs(seg).sum(axis=2) + 1e-6).all()), "chunk %d: %g" % (k, err.max())


# ------------------------------------------------------------------------------------------------ slab finalize
# The smallest shapes the sliding conv takes with fused statistics (slide_conv_plan wants 128 units: H / 8 x W / 32 columns
# x D / 4 slices).  n = 1: 130 workgroups -> 520 (workgroup, wave) pairs per channel, lanes 0-7 have nine, the others
# eight; n = 2: tests/test_gpu_s1_routing.py's slide32_stats (128 workgroups per 32-channel slice: eight pairs per lane); the
# last has one workgroup per CU, 1024 pairs = sixteen per lane, the whole batch (SLAB_BATCH) with nothing guarded away.
# No sliding conv has more workgroups than CUs, so no lane ever takes a second batch there.
SLAB_CASES = [(1, 32, 32, (52, 40, 64)), (2, 32, 64, (16, 32, 64)), (2, 32, 32, (32, 64, 64))]


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("n,cin,cout,dims", SLAB_CASES, ids=["n1_ragged", "n2", "n2_full_batch"])
def test_slab_finalize_vs_separate_pass(n, cin, cout, dims, dt):
    g = torch.Generator().manual_seed(n + cin + cout + sum(dims))
    xv = torch.randn((n, cin) + dims, generator=g)
    wt = torch.randn(cout, cin, 3, 3, 3, generator=g) * (1.0 / (27 * cin) ** 0.5)
    b = torch.randn(cout, generator=g)
    x = ops.as_input(xv.to(DEV), dt)
    pw = ops.pack_weight(wt.to(DEV), N.ROLE_CONV_FWD, dt, 1)
    y, mean, scale = _logged(["conv3_s1_slide32<stats>", "stats_slab_finalize"], ops.conv_fwd_in, x, pw, b.to(DEV), cout, 3, 1)
    m2, s2 = ops.in_stats(y)
    # not equal: the conv's sums are taken over the fp32 accumulators before they are rounded to the storage type
    assert (mean.double() - m2.double()).abs().max().item() < 1e-5
    assert (scale.double() - s2.double()).abs().max().item() < 1e-4


# ------------------------------------------------------------------------------------------------ weight-gradient slab sums
STAGED3, STAGED1 = "wgrad_staged_mfma<27,32>", "wgrad_staged_mfma<1,256>"
# (cin, cout, k, stride, n, output extents, slabs).  The staged kernel writes min(1024 / channel pairs, positions / 32)
# slabs (k = 1: four per workgroup of 256 positions); odd input extents keep the stride-2 tile kernels out.
_SMALL = [((1, 4, 8), 1), ((1, 7, 9), 2), ((2, 9, 12), 7), ((2, 8, 16), 8), ((3, 9, 10), 9), ((3, 8, 16), 12),
          ((3, 11, 32), 33)]
WG_CASES = {
    # four chunk lanes, batches of eight groups of four slabs: 33 slabs = two groups and a left-over slab on lane 0;
    # 170 slabs (64 x 96 channels: too many outputs for the 8-lane form) = 42 / 43 per lane, past the batch of 32
    "wgrad_reduce<64>": [(32, 32, 3, 2, 1, od, s) for od, s in _SMALL] + [(64, 96, 3, 2, 1, (9, 19, 32), 170)],
    # wgrad_reduce_launch gives this form 128 slabs or more, so 1, 2, 7, 8, 9 cannot reach it.  32 chunk lanes: 128 = one
    # group per lane, 129 / 161 = left-over slabs on some lanes, 1023 = seven groups + 3 (lane 31: + 2), 1200 = 37 / 38
    # slabs per lane, past the batch of 32
    "wgrad_reduce<8>": [(32, 32, 3, 2, 1, (15, 17, 16), 128), (32, 32, 3, 2, 1, (3, 25, 55), 129),
                        (32, 32, 3, 2, 1, (7, 23, 32), 161), (32, 32, 3, 2, 1, (31, 33, 32), 1023),
                        (32, 32, 1, 1, 2, (30, 32, 40), 1200)],
    # slabs in eights, then fours, then singly
    "wgrad_reduce_tiled<true>": [(128, 128, 3, 2, 1, od, s) for od, s in _SMALL],
}
WG_PARAMS = [pytest.param(name, case, id="%s-%d" % (name.split("_", 1)[1], case[6]))
             for name, cases in WG_CASES.items() for case in cases]


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("reduce_name,case", WG_PARAMS)
def test_wgrad_slab_sums_lattice_exact(reduce_name, case, dt):
    cin, cout, k, stride, n, od, slabs = case
    xd = tuple((o - 1) * stride + 1 for o in od)
    g = torch.Generator().manual_seed(cin + cout + sum(od) + slabs)
    xv, gy = _lattice((n, cin) + xd, g), _lattice((n, cout) + od, g)
    assert 4 * n * od[0] * od[1] * od[2] < 2 ** 24      # every partial sum is an integer fp32 holds exactly
    x, gyd = ops.as_input(xv.to(DEV), dt), ops.as_input(gy.to(DEV), dt)
    # the plan query: the scratch is `groups` slabs of taps x Cin x Cout floats
    dx, ddy = N.desc(x), N.desc(gyd)
    nbytes = N.lib.ru3d_conv3d_wgrad_workspace_bytes(N.ref(dx), N.ref(ddy), k, stride, N.dtype_code(dt))
    assert nbytes == slabs * k ** 3 * cin * cout * 4, "the plan has %g slabs, this case is for %d" % (
        nbytes / (k ** 3 * cin * cout * 4.0), slabs)
    gw = _logged([STAGED3 if k == 3 else STAGED1, reduce_name], ops.conv_wgrad, x, gyd, k, stride).cpu()
    ref = _wgrad_ref(xv, gy, k, stride, torch.float64).float()
    assert gw.shape == ref.shape
    bad = int((gw != ref).sum())
    assert torch.equal(gw, ref), "%d of %d entries differ, first at %s" % (bad, ref.numel(), (gw != ref).nonzero()[0].tolist())


# ------------------------------------------------------------------------------------------------ the head's finalize
# head_bwd_kernel writes one row of 4 Cin + 4 floats per workgroup, min(2048, positions / (4 x 256 / (Cin / 8))) of them,
# into the caller's scratch; head_bwd_finalize_kernel gives every value a wave: lane l adds rows l, l + 64, ... ascending in
# double (one guarded batch of 32: 2048 rows are the most there can be), then wave_sum_d's butterfly.  Rows: one; below, at
# and above the 64 lanes; two per lane and a ragged third; 2047 and 2048, the whole batch.
HEAD_CASES = [(1, (1, 1, 200), 1), (1, (1, 9, 28 * 64), 63), (1, (1, 1, 64 * 256), 64), (1, (1, 5, 3330), 66),
              (2, (1, 20, 1000), 157), (1, (1, 2047, 256), 2047), (2, (4, 256, 256), 2048)]


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("n,dims,rows", HEAD_CASES, ids=["r%d" % c[2] for c in HEAD_CASES])
def test_head_bwd_finalize_order(n, dims, rows, dt):
    cin, cout = 32, 3
    positions = n * dims[0] * dims[1] * dims[2]
    assert min(2048, -(-positions // 256)) == rows      # Cin = 32: 64 voxel lanes x 4 positions each per workgroup
    g = torch.Generator().manual_seed(positions)
    x = ops.as_input((torch.randn((n, cin) + dims, generator=g) + 0.5).to(DEV), dt)
    gy = N.to_ndhwc((torch.randn((n, cout) + dims, generator=g) * 1e-2 + 3e-3).to(DEV))
    wt = (torch.randn(cout, cin, 1, 1, 1, generator=g) * 0.3).to(DEV)
    with ops.launch_log() as log:
        out = ops.head_bwd(x, gy, wt, True)
    assert out is not None and log.names == ["head_bwd", "head_bwd_finalize"], log.names
    _, dw, db = out
    torch.cuda.synchronize()
    row = 4 * cin + 4
    ws = N.workspace(rows * row * 4, DEV)      # the scratch the call used: one buffer per (device, stream)
    part = _floats(ws, 0, rows * row).reshape(rows, row).astype(np.float64)
    lanes = np.zeros((64, row), dtype=np.float64)
    for b in range(rows):
        lanes[b % 64] += part[b]
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[idx ^ o]
    want = lanes[0].astype(np.float32)
    assert np.array_equal(_bits(dw.cpu().numpy().reshape(cout, cin)), _bits(want[:4 * cin].reshape(4, cin)[:cout])), "dW"
    assert np.array_equal(_bits(db.cpu().numpy()), _bits(want[4 * cin:4 * cin + cout])), "db"
