"""What the boundary term costs next to the Hybird loss, and what the fused signed-distance stage saves over composing it
from the evaluation kernels: on channel-last float32 logits of 2 x 3 x 128^3 (the layout the network hands over), HIP-event
times of
  * loss.HybirdLoss forward + backward,
  * loss.HybirdBoundaryLoss forward + backward,
  * the signed-distance stage alone (loss.signed_distance_map: all 2 x 2 maps in one launch sequence),
  * the composed route of the same maps: for each (sample, class) two morphology.pack and two distance.edt_squared calls
    (float64, one mask a call) plus the torch glue for sign, square root and the degenerate rule,
  * the composed boundary term forward + backward: those maps, torch.softmax, the weighted mean, autograd,
for three label patterns: phantom blobs, class 2 present as a single voxel (the longest scans), class 2 absent.  Median of
REPS passes after WARM warm-up passes, each pass between two events on the stream.  The fused and the composed maps are
compared element by element before anything is timed.  Prints one line per figure and a JSON summary line, and writes the
same text to profiles/boundary_loss_2x128.txt."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "3d-unet-renal-anatomy-extraction_amd"))
import numpy as np, torch, loss as L, morphology, distance
from oracle import unet_oracle as O
dev = torch.device("cuda:0")
SHAPE, REPS, WARM = (2, 3, 128, 128, 128), 15, 3
CLASSES = (1, 2)
OUT = os.path.join(ROOT, "profiles", "boundary_loss_2x128.txt")
lines = []


def say(text):
    print(text); lines.append(text)


def timed(fn):
    """Median milliseconds of REPS calls, each between two events; WARM calls first (code objects, allocator, workspace)."""
    out = []
    for i in range(WARM + REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out[WARM:]))


def composed_maps(y):
    """phi (N, K, A, B, Z) float32 from the evaluation kernels: what a user of the parent commit would have written."""
    maps = []
    for n in range(y.shape[0]):
        for q in CLASSES:
            lab = y[n]
            g = lab == q
            to_fg = distance.edt_squared(morphology.pack(lab, 'eq', q))
            to_bg = distance.edt_squared(morphology.pack((~g).to(torch.uint8)))
            phi = torch.where(g, -(to_bg.sqrt().float() - 1.0), to_fg.sqrt().float())
            maps.append(torch.where(torch.isfinite(phi), phi, torch.zeros_like(phi)))     # empty or full: no map
    return torch.stack(maps).view((y.shape[0], len(CLASSES)) + tuple(y.shape[1:]))


def composed_term(x, y):
    p = torch.softmax(x, dim=1)[:, list(CLASSES)]
    return (p * composed_maps(y)).sum((0, 2, 3, 4)).sum() / (len(CLASSES) * x.shape[0] * x[0, 0].numel())


def fwd_bwd(crit, x, y):
    x.grad = None
    crit(x, y).backward()


x = torch.randn(SHAPE, generator=torch.Generator().manual_seed(0)).contiguous(memory_format=torch.channels_last_3d).to(dev)
x.requires_grad_(True)
blobs = O.phantom_labels(SHAPE[0], SHAPE[2:], SHAPE[1]).to(torch.uint8)
single = torch.where(blobs == 2, torch.zeros_like(blobs), blobs)
absent = single.clone()
single[:, 5, 7, 9] = 2
patterns = {"phantom blobs": blobs.to(dev), "class 2 a single voxel": single.to(dev), "class 2 absent": absent.to(dev)}
say("logits %s float32 channel-last, uint8 labels, classes %s; HIP-event times, median of %d passes after %d warm-up passes"
    % (SHAPE, CLASSES, REPS, WARM))
summary = {}
for name, y in patterns.items():
    fused = L.signed_distance_map(y, SHAPE[1], CLASSES)
    same = bool(torch.equal(fused, composed_maps(y)))
    ms = {"HybirdLoss fwd+bwd": timed(lambda: fwd_bwd(L.HybirdLoss(), x, y))}
    crit = L.HybirdBoundaryLoss()
    ms["HybirdBoundaryLoss fwd+bwd"] = timed(lambda: fwd_bwd(crit, x, y))
    ms["signed-distance stage, fused"] = timed(lambda: L.signed_distance_map(y, SHAPE[1], CLASSES))
    ms["signed-distance stage, composed"] = timed(lambda: composed_maps(y))
    ms["boundary term fwd+bwd, fused"] = timed(lambda: fwd_bwd(L.BoundaryLoss(classes=CLASSES), x, y))
    ms["boundary term fwd+bwd, composed"] = timed(lambda: fwd_bwd(composed_term, x, y))
    L.raise_on_bad_labels(wait=True)
    say("%s (fused maps == composed maps: %s)" % (name, same))
    for k, t in ms.items():
        say("  %-36s %9.3f ms" % (k, t))
    say("  %-36s %9.3f ms" % ("added by the boundary term", ms["HybirdBoundaryLoss fwd+bwd"] - ms["HybirdLoss fwd+bwd"]))
    say("  %-36s %9.2f x" % ("composed / fused, maps", ms["signed-distance stage, composed"] / ms["signed-distance stage, fused"]))
    summary[name] = dict({k: round(v, 3) for k, v in ms.items()}, maps_equal=same)
say(json.dumps({"shape": SHAPE, "reps": REPS, "warmup": WARM, "ms": summary}))
out = os.environ.get("RU3D_OUT")
path = os.path.join(out, os.path.basename(OUT)) if out else OUT
with open(path, "w") as f:
    f.write("\n".join(lines) + "\n")
