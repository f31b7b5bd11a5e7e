#!/usr/bin/env python3
"""Golden fixture of the plain 3D U-Net from the *reference itself*: reference network.py `Unet` (:470-565) with its own
default blocks - ConvBlockStack encoders / decoders (:153-199), MaxPoolBlock pooling (:452-463) - on the channel plan
generate_paired_features2(2, 8), with reference loss.py `HybirdLoss`, torch CPU fp32, one forward + backward in train
mode (every Dropout3d.p = 0) on the G1-style synthetic 32^3 case.  Only tensors are stored.

The ~2.4 MB of tensors are split over three files of under 1 MiB each, to keep every file added to the history small:
g13_plain.npz (x, y, weights, loss), g13_plain_logits.npz (logits) and g13_plain_grads.npz (parameter gradients).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_plain.py
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as G  # noqa: E402  (loads the reference's network.py / loss.py)


def main():
    x = G.synth_image((2, 1, 32, 32, 32), 77)
    y = G.phantom_labels(2, (32, 32, 32), 3)
    torch.manual_seed(0)
    net = G.ref_network
    model = net.Unet(in_channels=1, out_channels=3, paired_features=net.generate_paired_features2(2, 8))
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout3d):
            m.p = 0.0
    model.train()
    main_part = {"x": x.numpy(), "y": y.numpy().astype(np.uint8)}
    for k, v in model.state_dict().items():
        main_part["w/" + k] = v.detach().numpy().copy()
    logits = model(x)
    loss = G.ref_loss.HybirdLoss(weight_v=[1, 10, 20])(logits, y)
    loss.backward()
    main_part["loss"] = np.float64(loss.item())
    grads = {}
    for k, p in model.named_parameters():
        assert p.grad is not None, k
        grads["g/" + k] = p.grad.numpy().copy()
    nparam = sum(p.numel() for p in model.parameters())
    print("plain", float(loss), tuple(logits.shape), nparam, "parameters in", len(grads), "tensors; labels",
          sorted(int(v) for v in y.unique()))
    np.savez_compressed(os.path.join(G.OUT, "g13_plain.npz"), **main_part)
    np.savez_compressed(os.path.join(G.OUT, "g13_plain_logits.npz"), logits=logits.detach().numpy())
    np.savez_compressed(os.path.join(G.OUT, "g13_plain_grads.npz"), **grads)
    for name in ("g13_plain.npz", "g13_plain_logits.npz", "g13_plain_grads.npz"):
        size = os.path.getsize(os.path.join(G.OUT, name))
        assert size < (1 << 20), (name, size)
        print("wrote", name, size, "bytes")


if __name__ == "__main__":
    main()
