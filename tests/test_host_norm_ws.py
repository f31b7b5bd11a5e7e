"""The reduction workspace of csrc/norm.hip as a host contract (no device: ru3d_reduce_workspace_bytes is a pure query).

Python allocates by that value and api.hip sizes four fused entry points from it, so it is pinned to its closed form
2 * n * min(V, 4096) * C * 16 + n * C * 8 + 512 - the value of the commit before the layout got its struct (ReduceWs) -
and held above what the launches write: for every vector width pick_vec may choose, the end of the layout's last region.
`chanloop` and `ws_end` restate make_chanloop and ReduceWs; tests/test_gpu_chanloop.py runs the kernels on exactly these
sizes with sentinels on both sides."""
import ctypes

import pytest

import _native as N

FAKE = 0x10000      # a non-null, 16-byte aligned address: the query never dereferences it


def chanloop(V, c, vec, max_iters, n):
    """make_chanloop restated -> (G, Gb, vpb, span, chunks)"""
    G = c // vec
    Gb = min(G, 256)
    vpb = 256 // Gb
    gz = -(-G // Gb)
    iters = -(-(V * n * gz) // (vpb * 2048))
    iters = min(max(iters, 4), max_iters)
    span = vpb * iters
    chunks = -(-V // span)
    if chunks > 4096:
        span = -(-V // 4096)
        span = -(-span // vpb) * vpb
        chunks = -(-V // span)
    return G, Gb, vpb, span, chunks


def ws_end(n, c, V, vec):
    """ReduceWs restated: where its last region ends at width `vec` - the reduction partials (n * chunks * C pairs of
    doubles, 64 iterations at most), m12 rounded up to 256 bytes and, with dy_sum, the apply pass's partials (16
    iterations at most)."""
    chunks = chanloop(V, c, vec, 64, n)[4]
    chunks_a = chanloop(V, c, vec, 16, n)[4]
    m12 = -(-(n * c * 8) // 256) * 256
    return n * chunks * c * 16 + m12 + n * chunks_a * c * 16


def ws_need(n, c, V, itemsize):
    """ws_end maximised over the widths pick_vec may choose for elements of `itemsize` bytes"""
    return max(ws_end(n, c, V, vec) for vec in (8, 4, 2, 1) if vec * itemsize <= 16 and c % vec == 0)


def closed_form(n, c, V):
    return 2 * n * min(V, 4096) * c * 16 + n * c * 8 + 512


def _bytes(n, c, dims):
    t = N.Tensor(FAKE, n, dims[0], dims[1], dims[2], c, c, 0, 0)
    return int(N.lib.ru3d_reduce_workspace_bytes(ctypes.byref(t)))


# tests/test_gpu_chanloop.py's WS_CASES (their (2, 512, 8^3) is the benchmark's deepest level) and test_chunk_cap_respan,
# the benchmark's five levels, config 4's level 0
CASES = [(2, c, (1, 1, v)) for c in (8, 320) for v in (1, 2, 3, 5)] + [(1, 257, (66, 64, 64))] + \
    [(2, 32 << lv, (128 >> lv,) * 3) for lv in range(5)] + [(2, 30, (160, 160, 80))]


@pytest.mark.parametrize("n,c,dims", CASES, ids=lambda v: str(v).replace(" ", ""))
def test_reduce_workspace_bytes(n, c, dims):
    V = dims[0] * dims[1] * dims[2]
    got = _bytes(n, c, dims)
    assert got == closed_form(n, c, V)
    for vec in (8, 4, 2, 1):
        if c % vec == 0:
            assert got >= ws_end(n, c, V, vec), "width %d: the layout ends at %d of %d bytes" % (vec, ws_end(n, c, V, vec), got)


def test_null_tensor_needs_nothing():
    assert N.lib.ru3d_reduce_workspace_bytes(None) == 0
