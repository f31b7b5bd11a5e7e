#!/usr/bin/env python3
"""Golden fixture G14 of the ignore label from the *reference itself*.  The reference has no ignore label, but it fixes
the definition: the loss with an ignore label is the reference's loss applied to the counted voxels alone.  So the
voxels whose label is not 255 are gathered into one (1, C, M) batch, reference loss.py `HybirdLoss(weight_v=[1, 10, 20],
alpha=.9, beta=.1)`, `DiceLoss()`, `FocalLoss()` and `Dice()` run on it (torch CPU; the values in float32 as the
reference computes them, the logit gradients from a float64 run), and the gradients are scattered back with zeros at
the ignored voxels.  Two label maps: `y` with 255 on about 40 % of the voxels - one whole z-slab and every voxel of
class 2 in sample 1 among them - and `y1` with everything ignored except one voxel (M = 1).  Only tensors are stored.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_ignore.py
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as G  # noqa: E402  (loads the reference's loss.py)

IGNORE = 255
SHAPE = (2, 3, 9, 10, 12)


def losses():
    L = G.ref_loss
    return {"hybird": L.HybirdLoss(weight_v=[1, 10, 20], alpha=.9, beta=.1), "diceloss": L.DiceLoss(),
            "focal": L.FocalLoss(), "dice": L.Dice()}


def compacted(z, y, dtype):
    """The counted voxels as one (1, C, M) batch (a leaf that wants a gradient) and their (1, M) labels."""
    c = z.shape[1]
    keep = (y != IGNORE).reshape(-1)
    rows = z.movedim(1, -1).reshape(-1, c)[keep]
    return rows.t()[None].to(dtype).contiguous().requires_grad_(True), y.reshape(-1)[keep][None].long(), keep


def run(z, y, tag, out):
    c = z.shape[1]
    for name, crit in losses().items():
        x32, t, keep = compacted(z, y, torch.float32)
        value = crit(x32, t)
        x64, t, _ = compacted(z, y, torch.float64)
        crit(x64, t).backward()
        grad = torch.zeros(keep.numel(), c, dtype=torch.float64)
        grad[keep] = x64.grad[0].t()
        grad = grad.reshape(z.shape[0], *z.shape[2:], c).movedim(-1, 1).contiguous()
        out["%s/%s/value" % (tag, name)] = np.float64(value.item())
        out["%s/%s/grad" % (tag, name)] = grad.numpy()
        print(tag, name, "M =", int(keep.sum()), "value %.8f" % value.item(), "max|grad| %.3g" % grad.abs().max().item())


def main():
    n, c, d, h, w = SHAPE
    g = torch.Generator().manual_seed(1414)
    z = torch.randn(SHAPE, generator=g) * 2.0
    y = torch.randint(0, c, (n, d, h, w), generator=g)
    y[torch.rand((n, d, h, w), generator=g) < 0.19] = IGNORE
    y[:, 4] = IGNORE                          # one whole z-slab
    y[1][y[1] == 2] = IGNORE                  # class 2 of sample 1 lies under ignored voxels only
    y1 = torch.full((n, d, h, w), IGNORE, dtype=torch.int64)
    y1[1, 7, 3, 5] = 1                        # M = 1
    share = float((y == IGNORE).float().mean())
    assert 0.35 < share < 0.45, share
    out = {"z": z.numpy(), "y": y.numpy().astype(np.uint8), "y1": y1.numpy().astype(np.uint8)}
    run(z, y, "a", out)
    run(z, y1, "one", out)
    path = os.path.join(G.OUT, "g14_ignore.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < (1 << 20), size
    print("wrote g14_ignore.npz", size, "bytes; ignored share %.3f" % share)


if __name__ == "__main__":
    main()
