#!/usr/bin/env python3
"""Golden fixture G11: what the reference's `case_plt` hands to its `grid_plt`, on a small synthetic case.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_visualize.py

The reference's visualize.py is imported by path and its `grid_plt` is replaced by a recorder, so nothing is drawn; for
every call the panels and the value ranges are stored (g11_visualize.npz) together with the case and the arguments.
Only arrays are stored; no source text of the reference enters the repository.
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF  # noqa: E402  (the reference checkout, RU3D_REFERENCE)

CALLS = [(0.5, 0, False, False), (0.25, 1, False, False), (0.7, 2, False, False), (0.5, 2, True, True),
         (0.3, 0, True, False), (0.55, 1, True, True)]


def main():
    import matplotlib
    matplotlib.use("Agg")
    spec = importlib.util.spec_from_file_location("ref_visualize", os.path.join(REF, "visualize.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    recorded = []
    ref.grid_plt = lambda grid_list, value_ranges=None: recorded.append((grid_list, value_ranges))
    rng = np.random.default_rng(11)
    image = rng.normal(size=(13, 10, 9, 2)).astype(np.float32)
    image[rng.random(image.shape) < 0.1] = 0.0
    label = rng.integers(0, 4, size=(13, 10, 9)).astype(np.uint8)
    pred = rng.integers(0, 3, size=(13, 10, 9)).astype(np.uint8)
    hot_label = np.eye(4, dtype=np.float32)[label]
    hot_pred = np.eye(5, dtype=np.float32)[pred]      # one channel more than the label: the pred loop counts the label's
    out = {"image": image, "label": label, "pred": pred, "calls": np.array(CALLS, dtype=np.float64)}
    for i, (pct, axi, hl, hp) in enumerate(CALLS):
        case = {"image": image, "label": hot_label if hl else label, "pred": hot_pred if hp else pred}
        ref.case_plt(case, slice_pct=pct, axi=axi, one_hot_label=bool(hl), one_hot_pred=bool(hp))
        grid, ranges = recorded[-1]
        assert len(grid) == 1
        out["n_%d" % i] = np.array(len(grid[0]))
        out["ranges_%d" % i] = np.array(ranges, dtype=np.float64)
        for j, panel in enumerate(grid[0]):
            out["panel_%d_%d" % (i, j)] = np.asarray(panel)
    np.savez_compressed(os.path.join(HERE, "g11_visualize.npz"), **out)
    print("wrote g11_visualize.npz:", len(CALLS), "calls")


if __name__ == "__main__":
    main()
