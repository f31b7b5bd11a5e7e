"""What the soft-clDice term costs next to the Hybird loss: forward plus backward of loss.HybirdLoss and of
loss.HybirdClDiceLoss for k = 3, 5 and 10 soft-skeleton iterations, on channel-last float32 logits of 2 x 3 x 128^3 (the
layout the network hands over) with phantom labels; median of REPS passes after a warm-up pass, timed between
synchronises.  Prints one line per loss and a JSON summary line, and writes the same text to
profiles/cldice_loss_2x128.txt."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "3d-unet-renal-anatomy-extraction_amd"))
import numpy as np, torch, loss as L
from oracle import unet_oracle as O
dev = torch.device("cuda:0")
SHAPE, REPS = (2, 3, 128, 128, 128), 9
OUT = os.path.join(ROOT, "profiles", "cldice_loss_2x128.txt")
lines = []


def say(text):
    print(text); lines.append(text)


def passes(crit, x, y):
    out = []
    for _ in range(REPS + 1):                          # pass 0 warms up: code objects, allocator, workspace
        x.grad = None
        torch.cuda.synchronize(); t0 = time.perf_counter()
        crit(x, y).backward()
        torch.cuda.synchronize(); out.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(out[1:]))


x = torch.randn(SHAPE, generator=torch.Generator().manual_seed(0)).contiguous(memory_format=torch.channels_last_3d).to(dev)
x.requires_grad_(True)
y = O.phantom_labels(SHAPE[0], SHAPE[2:], SHAPE[1]).to(dev)
ms = {"HybirdLoss": passes(L.HybirdLoss(), x, y)}
for k in (3, 5, 10):
    ms["HybirdClDiceLoss k=%d" % k] = passes(L.HybirdClDiceLoss(iterations=k), x, y)
L.raise_on_bad_labels(wait=True)
say("logits %s float32 channel-last, forward + backward, median of %d passes after a warm-up pass" % (SHAPE, REPS))
for name, t in ms.items():
    say("  %-24s %9.3f ms  (+%.3f ms)" % (name, t, t - ms["HybirdLoss"]))
say(json.dumps({"shape": SHAPE, "reps": REPS, "ms": {k: round(v, 3) for k, v in ms.items()}}))
out = os.environ.get("RU3D_OUT")
path = os.path.join(out, os.path.basename(OUT)) if out else OUT
with open(path, "w") as f:
    f.write("\n".join(lines) + "\n")
