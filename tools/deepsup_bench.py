"""What deep supervision costs, and what the fused multi-level loss saves over composing it from the single-level loss: at
2 x 3 x 128^3 with L = 4 supervised levels (128^3, 64^3, 32^3, 16^3; channel-last float32 logits - the layout the heads
write - and uint8 labels), HIP-event times of
  * loss.DeepSupervisionLoss(HybirdLoss) forward + backward: one sums launch, one finalize, one backward launch for all
    levels, the labels read in place,
  * the same value composed from L loss.HybirdLoss calls on loss.downsample_labels(y, l).contiguous(), weighted and summed
    with torch ops, forward + backward: three launches and one label copy per level plus the glue,
  * loss.HybirdLoss forward + backward on level 0 alone (what a net without deep supervision pays),
  * the captured training step (graph.GraphedTrainStep, optim.Adam) of the benchmark model ResUnet3D(4, 32, 1, 3), bf16
    storage, batch 2 x 128^3, with deep_supervision=4 + DeepSupervisionLoss and without + HybirdLoss.
The two loss routes are compared (value and every level's gradient) before anything is timed.  Timing: WARM warm-up passes,
then ROUNDS rounds that alternate between the candidates; a round times REPS passes of one candidate between two events
and takes their mean; the figure is the median over the rounds, the spread is (max - min) over the rounds.  Prints one line
per figure and a JSON summary line, and writes the same text to profiles/deepsup_loss_2x128.txt (or $RU3D_OUT)."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "3d-unet-renal-anatomy-extraction_amd"))
import numpy as np, torch, graph, loss as L, network, optim
from oracle import unet_oracle as O
dev = torch.device("cuda:0")
N, C, FULL, LEVELS = 2, 3, (128, 128, 128), 4
WARM, ROUNDS, REPS, STEP_REPS = 5, 7, 50, 10
OUT = os.path.join(ROOT, "profiles", "deepsup_loss_2x128.txt")
lines = []


def say(text):
    print(text, flush=True); lines.append(text)


def alternate(candidates, reps):
    """{name: (median ms per pass, spread ms)} of callables timed in alternating rounds."""
    for fn in candidates.values():
        for _ in range(WARM):
            fn()
    torch.cuda.synchronize()
    got = {k: [] for k in candidates}
    for _ in range(ROUNDS):
        for k, fn in candidates.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record(); b.synchronize()
            got[k].append(a.elapsed_time(b) / reps)
    return {k: (float(np.median(v)), float(max(v) - min(v))) for k, v in got.items()}


g = torch.Generator().manual_seed(0)
xs = []
for l in range(LEVELS):
    shape = tuple(s >> l for s in FULL)
    x = torch.randn((N,) + shape + (C,), generator=g).to(dev).permute(0, 4, 1, 2, 3)      # NDHWC memory
    xs.append(x.requires_grad_(True))
y = O.phantom_labels(N, FULL, C).to(torch.uint8).to(dev)
ws = L.deep_supervision_weights(LEVELS)
fused_crit = L.DeepSupervisionLoss(L.HybirdLoss())
base = L.HybirdLoss()


def clear():
    for x in xs:
        x.grad = None


def fused():
    clear()
    v = fused_crit(xs, y)
    v.backward()
    return v


def composed():
    clear()
    v = sum(w * base(x, L.downsample_labels(y, l).contiguous()) for l, (w, x) in enumerate(zip(ws, xs)))
    v.backward()
    return v


def level0():
    clear()
    v = base(xs[0], y)
    v.backward()
    return v


vf = float(fused().detach()); gf = [x.grad.clone() for x in xs]
vc = float(composed().detach()); gc = [x.grad.clone() for x in xs]
L.raise_on_bad_labels(wait=True)
worst = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(gf, gc))
say("logits %s float32 channel-last on %d levels, uint8 labels; weights %s" % ((N, C) + FULL, LEVELS, [round(w, 4) for w in ws]))
say("fused value %.9g, composed value %.9g, largest gradient difference %.3g of a level's maximum" % (vf, vc, worst))
assert abs(vf - vc) <= 2e-6 * max(1.0, abs(vc)) and worst <= 1e-5, "the two routes disagree"
say("HIP-event times per pass: median of %d alternating rounds of %d passes (training step: %d), %d warm-up passes; "
    "spread = max - min over the rounds" % (ROUNDS, REPS, STEP_REPS, WARM))
loss_ms = alternate({"fused DeepSupervisionLoss fwd+bwd": fused, "composed from 4 HybirdLoss fwd+bwd": composed,
                     "HybirdLoss on level 0 alone fwd+bwd": level0}, REPS)
for k, (t, s) in loss_ms.items():
    say("  %-40s %8.3f ms   (spread %.3f)" % (k, t, s))
f, c, z = (loss_ms[k][0] for k in loss_ms)
say("  %-40s %8.2f x" % ("composed / fused", c / f))
say("  %-40s %8.3f ms" % ("fused minus level 0 alone", f - z))
clear()
del gf, gc


def make_step(levels):
    torch.manual_seed(0)
    model = network.ResUnet3D(4, 32, 1, C, deep_supervision=levels).to(dev)
    network.set_compute_dtype(model, torch.bfloat16)
    model.train()
    crit = L.DeepSupervisionLoss(L.HybirdLoss()) if levels else L.HybirdLoss()
    step = graph.GraphedTrainStep(model, crit, optim.Adam(model.parameters(), lr=1e-4), warmup=2)
    return step


xin = O.synth_image((N, 1) + FULL, 1).to(dev)
steps = {"step, deep_supervision=0 + HybirdLoss": make_step(0), "step, deep_supervision=4 + DeepSupervisionLoss": make_step(LEVELS)}
step_ms = alternate({k: (lambda s=s: s(xin, y)) for k, s in steps.items()}, STEP_REPS)
L.raise_on_bad_labels(wait=True)
assert all(s.replays > 0 for s in steps.values())
for k, (t, s) in step_ms.items():
    say("  %-48s %8.3f ms   (spread %.3f)" % (k, t, s))
p, d = (step_ms[k][0] for k in step_ms)
say("  %-48s %8.3f ms   (%.1f %%)" % ("added by deep supervision", d - p, 100.0 * (d - p) / p))
say(json.dumps({"shape": (N, C) + FULL, "levels": LEVELS, "rounds": ROUNDS, "reps": REPS, "step_reps": STEP_REPS, "warmup": WARM,
                "loss_ms": {k: [round(t, 3), round(s, 3)] for k, (t, s) in loss_ms.items()},
                "step_ms": {k: [round(t, 3), round(s, 3)] for k, (t, s) in step_ms.items()}}))
for s in steps.values():
    s.release()
out = os.environ.get("RU3D_OUT")
path = os.path.join(out, os.path.basename(OUT)) if out else OUT
with open(path, "w") as fh:
    fh.write("\n".join(lines) + "\n")
