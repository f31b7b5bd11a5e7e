"""The plan of the strided, transposed and 1x1x1 convs (ConvDirectPlan, conv.h), seen through the library's pure host
queries (no device: the CU budget reads 256 there).  Per (samples, channels, extents, pitch, dtype, CU budget) case of the
sweep below: the kernel names ru3d_conv3d_plan_names reports for the five forms of the family - 3x3x3 and 1x1x1 stride-2
gather (x to half extents), 1x1x1 stride 1, 3x3x3 and 1x1x1 stride-2 transposed (x to doubled extents) - and what the
fused entry points of the LDS-DMA tile kernels answer: the pooling pair's `supported` and slab bytes, the input-gradient
pair's `supported`, the ConvTranspose + InstanceNorm workspace.

tests/golden/direct_plan_table.json was written by `python tests/test_host_direct_plan.py FILE` with the library of the
commit BEFORE the dispatch was folded into one plan.  The four figures are that library's own; for the names that commit
got the same query on top of its unchanged if-ladder, which ran dry and returned the name where it would have launched.
No budget had to be left out: that library answers all four without a fault.  The test asserts that the library
reproduces the table exactly: a digest of every (budget, dtype, samples, extents) block of the full sweep, and the rows
themselves for a thinned set (what to look at when a digest differs)."""
import ctypes
import hashlib
import json
import os
import sys

if __name__ == "__main__":
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_root, os.path.join(_root, "3d-unet-renal-anatomy-extraction_amd"), os.path.join(_root, "tests")]

import _native as N  # noqa: E402
from test_host_conv_plan import BUDGETS, CHANNELS, DTYPES, EXTENTS, FAKE, ROW_PAIRS as S1_ROW_PAIRS  # noqa: E402

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "direct_plan_table.json")

# the sweep of the stride-1 table plus the two pairs of the inner level boundaries' GPU cases
PAIRS = [(ci, co) for ci in CHANNELS for co in CHANNELS] + [(48, 96), (48, 32)]
ROW_PAIRS = S1_ROW_PAIRS | {(48, 96), (48, 32)}
# (k, stride, transposed, y extents from x extents) of the five forms
FORMS = [(3, 2, 0, "half"), (1, 2, 0, "half"), (1, 1, 0, "same"), (3, 2, 1, "double"), (1, 2, 1, "double")]


def _t(n, dims, c, ld):
    return N.Tensor(FAKE, n, dims[0], dims[1], dims[2], c, ld, 0, 0)


def plan_names(x, y, k, stride, transposed, dt):
    """the names string of one geometry; '' where the library refuses it"""
    buf = ctypes.create_string_buffer(256)
    rc = N.lib.ru3d_conv3d_plan_names(ctypes.byref(x), ctypes.byref(y), k, stride, transposed, dt, buf, len(buf))
    return buf.value.decode() if rc == 0 else ""


def _case(n, cin, cout, dims, pitch, dt):
    """the five names and four figures of one case: x has cin channels on `dims`, y cout channels on the half / same /
    doubled extents, both with pitch `pitch` x channels"""
    lib = N.lib
    ys = {"half": tuple((e - 1) // 2 + 1 for e in dims), "same": dims, "double": tuple(2 * e for e in dims)}
    x = _t(n, dims, cin, cin * pitch)
    y = {key: _t(n, ext, cout, cout * pitch) for key, ext in ys.items()}
    rx, rh, rd = ctypes.byref(x), ctypes.byref(y["half"]), ctypes.byref(y["double"])
    return ([plan_names(x, y[to], k, s, tr, dt) for k, s, tr, to in FORMS] +
            [int(lib.ru3d_conv3d_s2_pair_fwd_in_supported(rx, rh, rh, dt)),
             int(lib.ru3d_conv3d_s2_pair_fwd_in_workspace_bytes(rx, rh, dt)),
             int(lib.ru3d_conv3d_s2_dgrad_pair_supported(rx, rx, None, rd, dt)),
             int(lib.ru3d_convtranspose3d_k3s2p1_fwd_in_workspace_bytes(rx, rd, dt))])


def sweep():
    """-> (digests {block: sha1 of its rows}, rows {case: names and figures} of the thinned set)"""
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
                                # the f16 twin runs the same host code: its rows would repeat the bf16 ones
                                if ((cin, cout) in ROW_PAIRS and dt == N.BF16 and pitch == 1 and n == 2 and
                                        budget in (0, 208)):
                                    rows["%s c%d-%d" % (block, cin, cout)] = fig
                        digests[block] = h.hexdigest()[:16]
    finally:
        N.lib.ru3d_set_cu_budget(0)
    return digests, rows


def test_direct_plan_table_is_reproduced():
    want = json.load(open(TABLE))
    digests, rows = sweep()
    assert N.lib.ru3d_get_cu_budget() == 256
    assert sorted(rows) == sorted(want["rows"])
    wrong = {k: (rows[k], want["rows"][k]) for k in rows if rows[k] != want["rows"][k]}
    assert not wrong, "%d rows differ, e.g. %s" % (len(wrong), sorted(wrong.items())[:4])
    assert digests == want["digests"], sorted(k for k in digests if digests[k] != want["digests"].get(k))[:8]


if __name__ == "__main__":
    d, r = sweep()
    with open(sys.argv[1], "w") as f:
        json.dump({"digests": d, "rows": r}, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print(len(d), "blocks,", len(r), "rows")
