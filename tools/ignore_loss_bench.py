"""What the ignore label costs the softmax losses: on channel-last float32 logits of 2 x 3 x 128^3 (the layout the network
hands over) and int64 labels, HIP-event times of forward + backward, all in one run, of
  * loss.HybirdLoss() three times - the same plain loss under three names, timed like any other contender: the spread
    between them is what two figures of this file may differ by without meaning anything,
  * loss.HybirdLoss(ignore_label=255) with 0 %, 50 % and 95 % of the voxels ignored (drawn voxel by voxel, the pattern
    that splits the most waves),
  * loss.DeepSupervisionLoss(HybirdLoss) on L = 4 levels (128^3 .. 16^3) and loss.HybirdTopKLoss(k=10), each without the
    label and with it on the 50 % labels.
The ignore form moves the same bytes as the plain one (labels and logits are read, every gradient element is written) and
adds one compare per voxel; an ignored voxel skips its softmax.  The contenders are timed in alternating passes (A, B, C,
..., A, B, C, ...), each pass between two events on the stream, REPS passes each after WARM warm-up passes; median, minimum
and maximum are printed.  The ignore form is compared with its host twin on a small tensor before anything is timed.
Prints one line per figure and a JSON summary line, and writes the same text to profiles/ignore_loss_2x128.txt."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "3d-unet-renal-anatomy-extraction_amd"))
import numpy as np, torch, loss as L
from oracle import unet_oracle as O
dev = torch.device("cuda:0")
SHAPE, REPS, WARM, LEVELS, IGNORE = (2, 3, 128, 128, 128), 25, 5, 4, 255
OUT = os.path.join(ROOT, "profiles", "ignore_loss_2x128.txt")
lines = []


def say(text):
    print(text); lines.append(text)


def fwd_bwd(crit, x, y):
    for t in (x if isinstance(x, list) else [x]):
        t.grad = None
    crit(x, y).backward()


def one_pass(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record()
    b.synchronize()
    return a.elapsed_time(b)


def logits(shape, seed):
    x = torch.randn(shape, generator=torch.Generator().manual_seed(seed)).contiguous(memory_format=torch.channels_last_3d)
    return x.to(dev).requires_grad_(True)


def labels(share):
    y = O.phantom_labels(SHAPE[0], SHAPE[2:], SHAPE[1])
    if share:
        y[torch.rand(y.shape, generator=torch.Generator().manual_seed(7)) < share] = IGNORE
    return y.to(dev)


small = torch.randn((2, 3, 9, 10, 11), generator=torch.Generator().manual_seed(1))
small_y = torch.randint(0, 3, (2, 9, 10, 11), generator=torch.Generator().manual_seed(2))
small_y[torch.rand(small_y.shape, generator=torch.Generator().manual_seed(3)) < 0.4] = IGNORE
twin = float(L.DeepSupervisionLoss(L.HybirdLoss(ignore_label=IGNORE))([small.double()], small_y))
got = float(L.HybirdLoss(ignore_label=IGNORE)(small.to(dev), small_y.to(dev)))
same = abs(got - twin) <= 2e-6 * max(1.0, abs(twin))

x = logits(SHAPE, 0)
xs = [x] + [logits(SHAPE[:2] + tuple(s >> l for s in SHAPE[2:]), l) for l in range(1, LEVELS)]
y = {share: labels(share) for share in (0.0, 0.5, 0.95)}
plain, ign = L.HybirdLoss(), L.HybirdLoss(ignore_label=IGNORE)
contenders = {
    "HybirdLoss #1": (plain, x, y[0.0]),
    "HybirdLoss #2": (L.HybirdLoss(), x, y[0.0]),
    "HybirdLoss #3": (L.HybirdLoss(), x, y[0.0]),
    "HybirdLoss ignore  0 %": (ign, x, y[0.0]),
    "HybirdLoss ignore 50 %": (ign, x, y[0.5]),
    "HybirdLoss ignore 95 %": (ign, x, y[0.95]),
    "DeepSupervision L=4": (L.DeepSupervisionLoss(L.HybirdLoss()), xs, y[0.0]),
    "DeepSupervision L=4 ignore 50 %": (L.DeepSupervisionLoss(L.HybirdLoss(ignore_label=IGNORE)), xs, y[0.5]),
    "HybirdTopKLoss": (L.HybirdTopKLoss(k=10), x, y[0.0]),
    "HybirdTopKLoss ignore 50 %": (L.HybirdTopKLoss(k=10, ignore_label=IGNORE), x, y[0.5]),
}
times = {k: [] for k in contenders}
for i in range(WARM + REPS):
    for name, (crit, a, b) in contenders.items():
        t = one_pass(lambda: fwd_bwd(crit, a, b))
        if i >= WARM:
            times[name].append(t)
L.raise_on_bad_labels(wait=True)
say("logits %s float32 channel-last, int64 labels, ignore label %d; forward + backward, HIP-event times of %d alternating "
    "passes after %d warm-up passes" % (SHAPE, IGNORE, REPS, WARM))
say("ignore form on the device == host twin in float64 on a small tensor: %s (%.9g, %.9g)" % (same, got, twin))
ms = {}
for name, t in times.items():
    ms[name] = {"median": round(float(np.median(t)), 4), "min": round(float(np.min(t)), 4), "max": round(float(np.max(t)), 4)}
    say("  %-34s median %8.4f ms   min %8.4f   max %8.4f" % (name, ms[name]["median"], ms[name]["min"], ms[name]["max"]))
three = [ms["HybirdLoss #%d" % k]["median"] for k in (1, 2, 3)]
spread = (max(three) - min(three)) / min(three)
say("  spread of the plain HybirdLoss over its three entries: %.2f %% of the fastest median" % (100 * spread))
ratios = {}
for name, base in (("HybirdLoss ignore  0 %", min(three)), ("HybirdLoss ignore 50 %", min(three)),
                   ("HybirdLoss ignore 95 %", min(three)),
                   ("DeepSupervision L=4 ignore 50 %", ms["DeepSupervision L=4"]["median"]),
                   ("HybirdTopKLoss ignore 50 %", ms["HybirdTopKLoss"]["median"])):
    ratios[name] = round(ms[name]["median"] / base, 4)
    say("  %-34s %8.3f x its plain form" % (name, ratios[name]))
say(json.dumps({"shape": SHAPE, "levels": LEVELS, "reps": REPS, "warmup": WARM, "ms": ms, "plain_spread": round(spread, 4),
                "ratios": ratios, "equals_twin": same}))
out = os.environ.get("RU3D_OUT")
path = os.path.join(out, os.path.basename(OUT)) if out else OUT
with open(path, "w") as f:
    f.write("\n".join(lines) + "\n")
