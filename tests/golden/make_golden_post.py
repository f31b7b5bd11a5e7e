#!/usr/bin/env python3
"""Golden fixture G10: the reference's post-processing and evaluation helpers on a synthetic label volume.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_post.py

What runs from the reference: `create_sphere` and `post_transform` of nb_post.py (:81-112) and `evaluate_metrics` of
nb.py (:11-25), with the reference's own `transform.remove_small_region`.  The two notebooks cannot be imported - they
load checkpoints and data sets at import time - so they are parsed with `ast` and only the three function definitions
are executed, in a namespace that holds what those functions name (np, ndi, torch, remove_small_region).
Only arrays are stored (g10_post.npz); no source text of the reference enters the repository.

The volume (96 x 80 x 72, classes 0-3): a kidney-sized blob of class 1 with class 2 and class 3 inside (its foreground
component is far above the 10,000-voxel threshold), a small blob of class 1 around class 2 (below the threshold: its
class-1 voxels go, its class-2 core is painted back), a class-2 blob cut by the x = 95 face (the closing's border rule
clears what lies within the ball's reach of the face), pin holes in class 2 (the ball closes them), one-voxel spurs of
class 2 (the cross opens them away) and 0.3 % speckle of all classes.  `pred` / `label` for the metrics are the volume
and a shifted, re-speckled copy of it.  The scipy results of the four binary operations on masks of the same volume
are stored next to them for the numpy routes of transform.binary_*.
"""
import ast
import importlib.util
import os
import sys

import numpy as np
import scipy.ndimage as ndi
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF  # noqa: E402  (the reference checkout, RU3D_REFERENCE: the one every other fixture comes from)
SHAPE = (96, 80, 72)


def _functions(path, names):
    """The FunctionDef nodes `names` of a Python file, compiled on their own."""
    tree = ast.parse(open(path).read(), filename=path)
    picked = [node for node in tree.body if isinstance(node, ast.FunctionDef) and node.name in names]
    assert sorted(n.name for n in picked) == sorted(names), [n.name for n in picked]
    return compile(ast.Module(body=picked, type_ignores=[]), path, "exec")


def _reference():
    spec = importlib.util.spec_from_file_location("ref_transform", os.path.join(REF, "transform.py"))
    ref_transform = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref_transform)
    ns = {"np": np, "ndi": ndi, "torch": torch, "remove_small_region": ref_transform.remove_small_region}
    exec(_functions(os.path.join(REF, "nb_post.py"), ["create_sphere", "post_transform"]), ns)
    exec(_functions(os.path.join(REF, "nb.py"), ["evaluate_metrics"]), ns)
    return ns


def _ellipsoid(center, radii, wobble):
    x, y, z = np.ogrid[:SHAPE[0], :SHAPE[1], :SHAPE[2]]
    d = ((x - center[0]) / radii[0]) ** 2 + ((y - center[1]) / radii[1]) ** 2 + ((z - center[2]) / radii[2]) ** 2
    return d + wobble < 1


def synth_volume(seed=10):
    rng = np.random.RandomState(seed)
    wobble = ndi.gaussian_filter(rng.standard_normal(SHAPE), 4.0)
    wobble = 0.25 * wobble / np.abs(wobble).max()
    v = np.zeros(SHAPE, dtype=np.uint8)
    v[_ellipsoid((40, 40, 36), (28, 26, 24), wobble)] = 1            # the large component
    v[_ellipsoid((38, 42, 36), (15, 13, 12), wobble)] = 2
    v[_ellipsoid((50, 30, 30), (5, 5, 6), wobble)] = 3
    v[_ellipsoid((82, 12, 14), (11, 9, 10), wobble)] = 1             # below the threshold
    v[_ellipsoid((82, 12, 14), (6, 5, 5), wobble)] = 2
    v[_ellipsoid((93, 60, 50), (8, 10, 11), wobble)] = 2             # cut by the x = 95 face
    kd = v == 2
    v[kd & (rng.rand(*SHAPE) < 0.03)] = 1                            # pin holes in class 2
    v[20:38, 42, 36] = 2                                             # spurs, one voxel thick
    v[38, 42, 47:60] = 2
    v[60, 20:40, 60] = 2
    speckle = rng.rand(*SHAPE) < 0.003
    v[speckle] = rng.randint(1, 4, size=int(speckle.sum())).astype(np.uint8)
    return v


def synth_pair(volume, seed=11):
    rng = np.random.RandomState(seed)
    pred = np.roll(volume, (2, -1, 1), axis=(0, 1, 2))
    flip = rng.rand(*SHAPE) < 0.01
    pred[flip] = rng.randint(0, 4, size=int(flip.sum())).astype(np.uint8)
    return pred, volume.copy()


def main():
    ref = _reference()
    volume = synth_volume()
    out = {"input": volume}
    out["sphere"] = np.asarray(ref["create_sphere"]((7, 7, 7), (3, 3, 3), 4)).astype(np.uint8)
    out["post"] = ref["post_transform"](volume.copy())
    assert out["post"].dtype == np.uint8

    pred, label = synth_pair(volume)
    out["pred"], out["label"] = pred, label
    rows = []
    for c in range(1, int(label.max()) + 1):                         # the per-class loop of nb.py:28-36
        m = ref["evaluate_metrics"](torch.tensor((pred == c).astype(np.float32)), torch.tensor((label == c).astype(np.float32)))
        rows.append([m["dsc"], m["sen"], m["spe"], m["acc"]])
    out["metrics"] = np.array(rows, dtype=np.float64)                # [class - 1][dsc, sen, spe, acc]

    # scipy on masks of the same volume: what the numpy routes of transform.binary_* must return
    ball = out["sphere"].astype(bool)
    out["erosion_cross_fg"] = ndi.binary_erosion(volume > 0)
    out["dilation_ball_c3"] = ndi.binary_dilation(volume == 3, ball)
    out["closing_ball_c2"] = ndi.binary_closing(volume == 2, ball)
    out["opening_cross2_c2"] = ndi.binary_opening(volume == 2, iterations=2)
    out["closing_ball_c2_border1"] = ndi.binary_closing(volume == 2, ball, border_value=1)

    labels, count = ndi.label(volume > 0)
    sizes = np.bincount(labels.ravel())[1:]
    assert (sizes >= 10000).any() and ((sizes < 10000) & (sizes > 1000)).any(), sizes.max()
    assert (out["post"] != np.where(volume > 0, 1, 0)).any() and (out["post"] == 2).any()
    assert (volume[-3:] == 2).any() and not (out["post"][-3:] == 2).any()         # the border rule shows
    path = os.path.join(HERE, "g10_post.npz")
    np.savez_compressed(path, **out)
    print("%s: %d bytes, %d components, post changes %d voxels of max(input, 1)" % (
        path, os.path.getsize(path), count, int((out["post"] != np.minimum(volume, 2) * (volume > 0)).sum())))


if __name__ == "__main__":
    sys.exit(main())
