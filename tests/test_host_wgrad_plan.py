"""The weight-gradient plan (csrc/conv_mfma.hip wgrad_plan), seen through the library's pure host queries (no device: the
CU budget reads 256 there): the scratch figures of the four conv forms, the pair form's predicate and scratch for both
strides, the bias form's scratch, the ConvTranspose weight gradient's scratch and the planar-concat predicate, for every
(samples, channels, extents, pitch, dtype, CU budget) case of the sweep below.  The slab count differs between kernel
families and grids, so the eleven figures of a case together fingerprint the family and the decomposition the plan
chooses for it - and the figures themselves are what callers size pooled buffers from.

tests/golden/wgrad_plan_table.json was written by `python tests/test_host_wgrad_plan.py FILE` with the library of the
commit BEFORE the dispatch was folded into one plan; the test asserts that the library reproduces it exactly: a digest
of every (budget, dtype, samples, extents) block of the full sweep, and the rows themselves for a thinned set of channel
pairs (what to look at when a digest differs).  Only queries are called, with a fake pointer: nothing here may launch."""
import ctypes
import hashlib
import json
import os
import sys

if __name__ == "__main__":
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_root, os.path.join(_root, "3d-unet-renal-anatomy-extraction_amd")]

import _native as N  # noqa: E402

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wgrad_plan_table.json")

# tests/test_host_conv_plan.py's channel list and extents ...
CHANNELS = [32, 64, 96, 128, 192, 256, 512]
EXTENTS = ([(128 >> i,) * 3 for i in range(5)] + [(160 >> i, 160 >> i, 80 >> i) for i in range(5)] +
           [(192 >> i,) * 3 for i in range(6)] + [(7, 9, 13), (16, 40, 40), (16, 32, 56), (32, 48, 96), (20, 20, 10)])
# ... plus the stem (Cin = 1), the head (Cout = 2 .. 4) and a pair that is no multiple of 32 (the generic kernel)
EXTRA_PAIRS = [(1, 32), (1, 64), (32, 2), (32, 3), (32, 4), (64, 2), (64, 3), (64, 4), (30, 40)]
PAIRS = [(ci, co) for ci in CHANNELS for co in CHANNELS] + EXTRA_PAIRS
# no budget below 32 CUs: the library that wrote the table divides by zero there (see test_small_cu_budget below)
BUDGETS = [0, 208, 240]
DTYPES = [N.BF16, N.F16, N.F32]
ROW_PAIRS = {(c, c) for c in CHANNELS} | {(32, 64), (64, 32), (64, 128), (128, 64), (128, 256), (256, 128), (256, 512),
                                          (512, 256), (96, 192)} | set(EXTRA_PAIRS)
FAKE = 0x10000      # a non-null, 16-byte aligned address: the queries never dereference it


def _t(n, dims, c, ld):
    return N.Tensor(FAKE, n, dims[0], dims[1], dims[2], c, ld, 0, 0)


def _half(dims):
    """the output extents of a stride-2 conv (k = 1 or 3, pad = k // 2)"""
    return tuple((s - 1) // 2 + 1 for s in dims)


def _case(n, cin, cout, dims, pitch, dt):
    """the eleven figures of one case: x has cin channels, dy cout, both with pitch `pitch` x channels"""
    lib = N.lib
    x, dy, dyh = _t(n, dims, cin, cin * pitch), _t(n, dims, cout, cout * pitch), _t(n, _half(dims), cout, cout * pitch)
    up = _t(n, tuple(2 * s for s in dims), cout, cout * pitch)       # ConvTranspose: dy has twice x's extents
    rx, rdy, rdyh, rup = ctypes.byref(x), ctypes.byref(dy), ctypes.byref(dyh), ctypes.byref(up)
    return [int(lib.ru3d_conv3d_wgrad_workspace_bytes(rx, rdy, 3, 1, dt)),
            int(lib.ru3d_conv3d_wgrad_workspace_bytes(rx, rdyh, 3, 2, dt)),
            int(lib.ru3d_conv3d_wgrad_workspace_bytes(rx, rdy, 1, 1, dt)),
            int(lib.ru3d_conv3d_wgrad_workspace_bytes(rx, rdyh, 1, 2, dt)),
            int(lib.ru3d_conv3d_wgrad_pair_supported(rx, rdy, rdy, 1, dt)),
            int(lib.ru3d_conv3d_wgrad_pair_workspace_bytes(rx, rdy, rdy, 1, dt)),
            int(lib.ru3d_conv3d_wgrad_pair_supported(rx, rdyh, rdyh, 2, dt)),
            int(lib.ru3d_conv3d_wgrad_pair_workspace_bytes(rx, rdyh, rdyh, 2, dt)),
            int(lib.ru3d_conv3d_wgrad_bias_workspace_bytes(rx, rdy, 3, 1, dt)),
            int(lib.ru3d_convtranspose3d_k3s2p1_wgrad_workspace_bytes(rx, rup, dt)),
            int(lib.ru3d_planar_concat_supported(n, dims[0], dims[1], dims[2], cin, cout, dt))]


def sweep():
    """-> (digests {block: sha1 of its rows}, rows {case: figures} of the thinned set)"""
    digests, rows = {}, {}
    try:
        for budget in BUDGETS:
            assert N.lib.ru3d_set_cu_budget(budget) == 0
            for dt in DTYPES:
                for n in (1, 2, 3):
                    for dims in EXTENTS:
                        block = "b%d t%d n%d %dx%dx%d" % ((budget, dt, n) + dims)
                        h = hashlib.sha1()
                        for cin, cout in PAIRS:
                            for pitch in (1, 2):
                                fig = _case(n, cin, cout, dims, pitch, dt)
                                h.update(("%d %d %d %s\n" % (cin, cout, pitch, fig)).encode())
                                # the f16 twin runs the same host code, and fp32 differs only in the stem and head rows
                                if ((cin, cout) in ROW_PAIRS and pitch == 1 and n < 3 and budget == 0 and
                                        (dt == N.BF16 or (dt == N.F32 and (cin, cout) in EXTRA_PAIRS and n == 1))):
                                    rows["%s c%d-%d" % (block, cin, cout)] = fig
                        digests[block] = h.hexdigest()[:16]
    finally:
        N.lib.ru3d_set_cu_budget(0)
    return digests, rows


def test_wgrad_plan_table_is_reproduced():
    want = json.load(open(TABLE))
    digests, rows = sweep()
    assert N.lib.ru3d_get_cu_budget() == 256
    assert sorted(rows) == sorted(want["rows"])
    wrong = {k: (rows[k], want["rows"][k]) for k in rows if rows[k] != want["rows"][k]}
    assert not wrong, "%d rows differ, e.g. %s" % (len(wrong), sorted(wrong.items())[:4])
    assert digests == want["digests"], sorted(k for k in digests if digests[k] != want["digests"].get(k))[:8]


def test_small_cu_budget():
    """A CU budget below the channel-pair count (64 -> 192 = 12 pairs, 8 CUs) leaves the sliding kernel less than one
    workgroup per pair: the plan takes the next family (the tile kernel) instead of dividing by budget / pairs = 0, which
    killed the process (SIGFPE) before wgrad_plan.  The scratch is then whole slabs of 27 x 64 x 192 floats, no more than
    at the full budget, and the pair form (sliding kernel only at stride 1) is not offered."""
    lib, dims = N.lib, (128, 128, 128)
    x, dy = _t(1, dims, 64, 64), _t(1, dims, 192, 192)
    rx, rdy = ctypes.byref(x), ctypes.byref(dy)
    full = int(lib.ru3d_conv3d_wgrad_workspace_bytes(rx, rdy, 3, 1, N.BF16))
    try:
        assert lib.ru3d_set_cu_budget(8) == 0
        small = int(lib.ru3d_conv3d_wgrad_workspace_bytes(rx, rdy, 3, 1, N.BF16))
        pair = int(lib.ru3d_conv3d_wgrad_pair_supported(rx, rdy, rdy, 1, N.BF16))
    finally:
        lib.ru3d_set_cu_budget(0)
    print("64 -> 192 at 128^3: %d bytes under 8 CUs, %d at the full budget" % (small, full))
    assert small > 0 and small % (27 * 64 * 192 * 4) == 0 and small <= full
    assert pair == 0


if __name__ == "__main__":
    d, r = sweep()
    with open(sys.argv[1], "w") as f:
        json.dump({"digests": d, "rows": r}, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print(len(d), "blocks,", len(r), "rows")
