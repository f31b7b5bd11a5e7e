#!/usr/bin/env python3
"""Golden fixture G12: sliding-window inference with covering windows, Gaussian blending, mirror test-time
augmentation and a two-model ensemble.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_tta.py

The reference has no such mode, so the yardstick is the reference's NETWORK (its network.py, imported by make_golden.py,
cast to float64, torch CPU) under the merge rule of inference.py restated here in float64 numpy:
  * the case is zero-padded to at least the patch, (full - orig) // 2 rounded UP in front (transform.pad);
  * per axis n = ceil((L - P) * s / P) + 1 windows at (i * (L - P)) // (n - 1), loop order x outer, z inner;
  * every window is predicted once per subset of the mirror axes (by size, then lexicographic): the input is flipped,
    the softmax (sigmoid for one class) is flipped back;
  * a term is weighted by g_x[a] * g_y[j] * g_z[k], g[i] = exp(-0.5 * ((i - (P - 1) / 2) / (P / 8))**2) rounded to float32
    (the tables the device uses), or by 1; numerator and denominator are summed in float64 and divided;
  * the result is cropped where the padding put the case; the mask is the argmax (round half to even for one class).
Images, patches and the first weight set of cases `a`, `b`, `d` are READ from g6_predict.npz and not copied; the second
weight set of each case (the ensemble partner) is drawn here under a fixed seed and stored.  step_per_patch is 2.
Only tensors are stored (g12_tta.npz): float32 probabilities, uint8 masks, the window origins.
"""
import itertools
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as G  # noqa: E402  (loads the reference's network.py)

STEP = 2
SIGMA_SCALE = 0.125
CONFIGS = {                       # name: (weighting, mirror axes, number of weight sets)
    "cover_uniform": ("uniform", (), 1),
    "cover_gaussian": ("gaussian", (), 1),
    "cover_gaussian_m012": ("gaussian", (0, 1, 2), 1),
    "cover_gaussian_m02_ens": ("gaussian", (0, 2), 2),
}


def cover_origins(L, P, s):
    n = -((-(L - P) * s) // P) + 1
    return [0] if n == 1 else [(i * (L - P)) // (n - 1) for i in range(n)]


def profile(P):
    i = np.arange(P, dtype=np.float64)
    return np.exp(-0.5 * ((i - (P - 1) / 2.0) / (SIGMA_SCALE * P)) ** 2).astype(np.float32).astype(np.float64)


def subsets(axes):
    return [c for r in range(len(axes) + 1) for c in itertools.combinations(sorted(axes), r)]


def blend(image, models, ncls, patch, weighting, mirror_axes):
    orig = image.shape[:3]
    full = tuple(max(o, p) for o, p in zip(orig, patch))
    lo = tuple(-((o - f) // 2) for o, f in zip(orig, full))
    vol = np.zeros(full + (image.shape[3],), dtype=np.float64)
    vol[lo[0]:lo[0] + orig[0], lo[1]:lo[1] + orig[1], lo[2]:lo[2] + orig[2]] = image
    axes = [cover_origins(full[i], patch[i], STEP) for i in range(3)]
    w = np.ones(patch)
    if weighting == "gaussian":
        gx, gy, gz = (profile(p) for p in patch)
        w = gx[:, None, None] * gy[None, :, None] * gz[None, None, :]
    acc = np.zeros(full + (ncls,))
    cnt = np.zeros(full)
    x = torch.from_numpy(np.moveaxis(vol, -1, 0)[None].copy())               # [1, C, X, Y, Z]
    with torch.no_grad():
        for model in models:
            for ox in axes[0]:
                for oy in axes[1]:
                    for oz in axes[2]:
                        win = x[:, :, ox:ox + patch[0], oy:oy + patch[1], oz:oz + patch[2]]
                        for sub in subsets(mirror_axes):
                            dims = [2 + a for a in sub]
                            out = model(torch.flip(win, dims) if dims else win)
                            out = torch.sigmoid(out) if ncls == 1 else torch.softmax(out, dim=1)
                            out = torch.flip(out, dims) if dims else out
                            p = np.moveaxis(out[0].numpy(), 0, -1)
                            acc[ox:ox + patch[0], oy:oy + patch[1], oz:oz + patch[2]] += p * w[..., None]
                            cnt[ox:ox + patch[0], oy:oy + patch[1], oz:oz + patch[2]] += w
    prob = (acc / cnt[..., None])[lo[0]:lo[0] + orig[0], lo[1]:lo[1] + orig[1], lo[2]:lo[2] + orig[2]]
    mask = np.round(prob[..., 0]) if ncls == 1 else np.argmax(prob, axis=-1)
    origins = np.array([(a, b, c) for a in axes[0] for b in axes[1] for c in axes[2]])
    return prob, mask.astype(np.uint8), origins, float(cnt.min())


def margin(prob):
    if prob.shape[-1] == 1:
        return np.abs(prob[..., 0] - 0.5)
    s = np.sort(prob, axis=-1)
    return s[..., -1] - s[..., -2]


def main():
    g6 = np.load(os.path.join(G.OUT, "g6_predict.npz"))
    out = {}
    for tag in ("a", "b", "d"):
        patch = tuple(int(v) for v in g6[tag + "/patch"])
        _, pool, feat, ncls = (int(v) for v in g6[tag + "/meta"])
        image = g6[tag + "/image"].astype(np.float64)
        first = G.ref_network.ResUnet3D(num_pool=pool, num_features=feat, in_channels=1, out_channels=ncls)
        first.load_state_dict({k[len(tag) + 3:]: torch.from_numpy(g6[k]) for k in g6.files
                               if k.startswith(tag + "/w/")}, strict=True)
        torch.manual_seed(1200 + ord(tag))
        second = G.ref_network.ResUnet3D(num_pool=pool, num_features=feat, in_channels=1, out_channels=ncls)
        out.update(G.sd_np(second.state_dict(), tag + "/w2/"))
        models = [first.double().eval(), second.double().eval()]
        for name, (weighting, mirror_axes, count) in CONFIGS.items():
            prob, mask, origins, cmin = blend(image, models[:count], ncls, patch, weighting, mirror_axes)
            assert np.isfinite(prob).all()
            out["%s/%s/prob" % (tag, name)] = prob.astype(np.float32)
            out["%s/%s/mask" % (tag, name)] = mask
            out[tag + "/origins"] = origins
            m = margin(prob)
            print("g12/%s/%s: %d windows, classes %s, min cnt %.3g, margin < 1e-4: %.4f %%, < 1e-3: %.4f %%"
                  % (tag, name, len(origins), np.unique(mask).tolist(), cmin, 100 * (m < 1e-4).mean(),
                     100 * (m < 1e-3).mean()))
    np.savez_compressed(os.path.join(G.OUT, "g12_tta.npz"), **out)
    print("wrote g12_tta.npz")


if __name__ == "__main__":
    torch.set_num_threads(8)
    main()
