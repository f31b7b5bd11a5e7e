"""What the group loss costs next to the softmax loss it stands beside: on channel-last float32 logits of 2 x 3 x 128^3 (the
layout the network hands over) and uint8 labels, HIP-event times of
  * loss.HybirdLoss forward + backward, C = 3,
  * loss.GroupHybirdLoss forward + backward, K = 3, groups ((1, 2), (2,), (0,)), on the same two tensors.
Both read the logits and the labels twice and write the gradient once; the group loss spends an exp, a log1p and a division
per channel where the softmax spends an exp and a share of one logarithm.  The yardstick is HybirdLoss measured in the same
run, with a margin of 20 % for the extra transcendentals.  The two are timed in alternating passes (A, B, A, B, ...), each
pass between two events on the stream, REPS passes each after WARM warm-up passes; median, minimum and maximum are printed.
The group loss is compared with its host twin on a small tensor before anything is timed.  Prints one line per figure and
a JSON summary line, and writes the same text to profiles/group_loss_2x128.txt."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "3d-unet-renal-anatomy-extraction_amd"))
import numpy as np, torch, loss as L
from oracle import unet_oracle as O
dev = torch.device("cuda:0")
SHAPE, REPS, WARM = (2, 3, 128, 128, 128), 25, 5
GROUPS = ((1, 2), (2,), (0,))
MARGIN = 1.20
OUT = os.path.join(ROOT, "profiles", "group_loss_2x128.txt")
lines = []


def say(text):
    print(text); lines.append(text)


def fwd_bwd(crit, x, y):
    x.grad = None
    crit(x, y).backward()


def one_pass(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record()
    b.synchronize()
    return a.elapsed_time(b)


small = torch.randn((2, 3, 9, 10, 11), generator=torch.Generator().manual_seed(1))
small_y = torch.randint(0, 3, (2, 9, 10, 11), generator=torch.Generator().manual_seed(2))
twin = float(L.GroupHybirdLoss(GROUPS)(small.double(), small_y))
got = float(L.GroupHybirdLoss(GROUPS)(small.to(dev), small_y.to(dev)))
same = abs(got - twin) <= 2e-6 * max(1.0, abs(twin))

x = torch.randn(SHAPE, generator=torch.Generator().manual_seed(0)).contiguous(memory_format=torch.channels_last_3d).to(dev)
x.requires_grad_(True)
y = O.phantom_labels(SHAPE[0], SHAPE[2:], SHAPE[1]).to(torch.uint8).to(dev)
contenders = {"HybirdLoss fwd+bwd": L.HybirdLoss(), "GroupHybirdLoss fwd+bwd": L.GroupHybirdLoss(GROUPS)}
times = {k: [] for k in contenders}
for i in range(WARM + REPS):
    for name, crit in contenders.items():
        t = one_pass(lambda: fwd_bwd(crit, x, y))
        if i >= WARM:
            times[name].append(t)
L.raise_on_bad_labels(wait=True)
say("logits %s float32 channel-last, uint8 labels, groups %s; HIP-event times of %d alternating passes after %d warm-up passes"
    % (SHAPE, GROUPS, REPS, WARM))
say("group loss on the device == host twin in float64 on a small tensor: %s (%.9g, %.9g)" % (same, got, twin))
ms = {}
for name, t in times.items():
    ms[name] = {"median": round(float(np.median(t)), 4), "min": round(float(np.min(t)), 4), "max": round(float(np.max(t)), 4)}
    say("  %-26s median %8.4f ms   min %8.4f   max %8.4f" % (name, ms[name]["median"], ms[name]["min"], ms[name]["max"]))
ratio = ms["GroupHybirdLoss fwd+bwd"]["median"] / ms["HybirdLoss fwd+bwd"]["median"]
say("  %-26s %8.3f x  (yardstick: at most %.2f x; %s)" % ("GroupHybirdLoss / HybirdLoss", ratio, MARGIN,
                                                          "inside" if ratio <= MARGIN else "MISSED"))
say(json.dumps({"shape": SHAPE, "groups": GROUPS, "reps": REPS, "warmup": WARM, "ms": ms, "ratio": round(ratio, 4),
                "margin": MARGIN, "inside_margin": ratio <= MARGIN, "equals_twin": same}))
out = os.environ.get("RU3D_OUT")
path = os.path.join(out, os.path.basename(OUT)) if out else OUT
with open(path, "w") as f:
    f.write("\n".join(lines) + "\n")
