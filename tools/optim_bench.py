"""What the optimizer part of a training step costs on the parameter set of the benchmark model, ResUnet3D(4, 32, 1, 3):
optim.Adam, optim.AdamW and optim.SGD(momentum 0.99, Nesterov, weight decay 3e-5), each without and with max_grad_norm = 12,
next to torch.optim.SGD + torch.nn.utils.clip_grad_norm_ (what a user of the parent commit falls back to for the
nnU-Net / KiTS19 recipe).

Two figures per fused variant, both HIP-event times, median of REPS samples after WARM warm-up samples:
  * kernels: the launches of one step on tables that are already on the device (the norm's two launches when clipping, then
    the update), BURST steps enqueued back to back between two events, divided by BURST - the device time, which is what a
    replayed hipGraph of the step pays;
  * step():  one optimizer.step() between two events with the stream drained in front of it - the eager call as a training
    loop issues it, host work (table fill, one 40-byte row per parameter, its upload) included.
The torch route has only the second form.  The yardstick is ru3d_adam_multi on the same table: its `kernels` figure is
measured SPREAD times, each time on a freshly built optimizer, and the spread of those medians is printed - a new rule that is slower
than Adam by more than that is a finding.  Gradients are one real backward pass of the model (so the parameters without a
gradient are the real ones), scaled to a norm of about 30 so that the clip bites.  Prints one line per figure and a JSON
summary line, and writes the same text to profiles/optim_recipe.txt."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "3d-unet-renal-anatomy-extraction_amd"))
import numpy as np, torch, _native as N, loss as L, network, optim
from oracle import unet_oracle as O
dev = torch.device("cuda:0")
REPS, WARM, BURST, SPREAD = 31, 5, 20, 5
MAX_NORM = 12.0
OUT = os.path.join(ROOT, "profiles", "optim_recipe.txt")
lines = []


def say(text):
    print(text); lines.append(text)


def median_ms(fn, per=1, drain=False):
    out = []
    for i in range(WARM + REPS):
        if drain:
            torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / per)
    return float(np.median(out[WARM:]))


torch.manual_seed(0)
model = network.ResUnet3D(4, 32, 1, 3).to(dev)
network.set_compute_dtype(model, torch.bfloat16)
model.train()
x = O.synth_image((1, 1, 64, 64, 64), 1).to(dev)
y = O.phantom_labels(1, (64, 64, 64), 3).to(dev)
L.HybirdLoss()(model(x), y).backward()
params = list(model.parameters())
with_grad = [p for p in params if p.grad is not None]
gen = torch.Generator(device=dev).manual_seed(1)
count = sum(p.numel() for p in with_grad)
for p in with_grad:
    p.grad = (30.0 / count ** 0.5) * torch.randn(p.shape, generator=gen, device=dev)
grads = {p: p.grad.clone() for p in with_grad}
weights = {p: p.detach().clone() for p in params}
say("ResUnet3D(4, 32, 1, 3): %d parameter tensors, %d with a gradient, %.2f M elements with a gradient (%.1f MB a float32 "
    "stream); HIP-event times, median of %d after %d warm-up; kernels: %d steps back to back / %d"
    % (len(params), len(with_grad), count / 1e6, count * 4 / 1e6, REPS, WARM, BURST, BURST))


def reset():
    with torch.no_grad():
        for p in params:
            p.copy_(weights[p])
    for p in with_grad:
        p.grad = grads[p]


def kernels_of(opt):
    """The launches of one eager step of a fused optimizer on its own device tables (filled by the step before)."""
    plan, group = opt._plans[(0, False)], opt.param_groups[0]
    bufs = opt._clip.get(False)

    def run():
        N.note_device(dev)
        coef = None
        if bufs is not None:
            N.check(N.lib.ru3d_grad_sumsq(N.ptr(plan.table), N.ptr(plan.block_map), plan.nblocks, optim._CHUNK,
                                          N.ptr(bufs["partials"]), N.stream()), "grad_sumsq")
            N.check(N.lib.ru3d_grad_norm_finish(N.ptr(bufs["partials"]), plan.nblocks, 1.0, None, opt.max_grad_norm,
                                                N.ptr(bufs["norm"]), N.stream()), "grad_norm_finish")
            coef = bufs["norm"][1:]
        opt._launch(plan, group, 2.0, 1.0, coef)

    def burst():
        for _ in range(BURST):
            run()
    return burst


FUSED = [("Adam", lambda mgn: optim.Adam(params, lr=1e-4, max_grad_norm=mgn), 7),
         ("AdamW", lambda mgn: optim.AdamW(params, lr=1e-4, max_grad_norm=mgn), 7),
         ("SGD nesterov", lambda mgn: optim.SGD(params, 1e-3, momentum=0.99, nesterov=True, weight_decay=3e-5,
                                                max_grad_norm=mgn), 5)]
result = {"kernels": {}, "step": {}}
yard = []
for round_no in range(SPREAD):
    for name, make, _streams in FUSED:
        for mgn in (None, MAX_NORM):
            if round_no > 0 and not (name == "Adam" and mgn is None):
                continue
            reset()
            opt = make(mgn)
            opt.step(); opt.step()                       # state and tables exist
            key = name + (" + max_grad_norm" if mgn is not None else "")
            k_ms = median_ms(kernels_of(opt), per=BURST)
            if name == "Adam" and mgn is None:
                yard.append(k_ms)
            if round_no == 0:
                result["kernels"][key] = k_ms
                result["step"][key] = median_ms(opt.step, drain=True)
                if mgn is not None:
                    norm = float(opt.last_grad_norm)
                    result.setdefault("norm", {})[key] = norm
            torch.cuda.synchronize()
            del opt
reset()
t_opt = torch.optim.SGD(params, 1e-3, momentum=0.99, nesterov=True, weight_decay=3e-5)


def torch_route_inner():
    torch.nn.utils.clip_grad_norm_(params, MAX_NORM)
    t_opt.step()


# the gradient clones are made outside the timed region: only clip + step are between the events
def torch_sample():
    out = []
    for i in range(WARM + REPS):
        for p in with_grad:
            p.grad = grads[p].clone()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); torch_route_inner(); b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out[WARM:]))


result["step"]["torch.optim.SGD nesterov + torch clip_grad_norm_"] = torch_sample()
reset()
for p in with_grad:
    p.grad = grads[p].clone()
result["step"]["torch.optim.SGD nesterov, no clip"] = median_ms(t_opt.step, drain=True)

say("kernels (device time of one step's launches; float32 streams touched per element, + 1 read when clipping):")
streams_of = {name: n for name, _, n in FUSED}
for k, v in result["kernels"].items():
    n = streams_of[k.replace(" + max_grad_norm", "")] + (1 if "max_grad_norm" in k else 0)
    say("  %-34s %8.4f ms   %d streams, %6.2f TB/s" % (k, v, n, n * count * 4 / (v * 1e-3) / 1e12))
say("  %-34s %8.4f .. %8.4f ms over %d measurements on fresh optimizers (spread %.1f %%)"
    % ("Adam, run to run", min(yard), max(yard), SPREAD, 100.0 * (max(yard) - min(yard)) / min(yard)))
say("step() (eager call, host work included):")
for k, v in result["step"].items():
    say("  %-50s %8.4f ms" % (k, v))
for k, v in result.get("norm", {}).items():
    say("gradient norm seen by %s: %.6f (max_grad_norm %g)" % (k, v, MAX_NORM))
say(json.dumps({"elements": count, "reps": REPS, "warmup": WARM, "burst": BURST,
                "kernels_ms": {k: round(v, 4) for k, v in result["kernels"].items()},
                "adam_kernels_ms_runs": [round(v, 4) for v in yard],
                "step_ms": {k: round(v, 4) for k, v in result["step"].items()}}))
out = os.environ.get("RU3D_OUT")
path = os.path.join(out, os.path.basename(OUT)) if out else OUT
with open(path, "w") as f:
    f.write("\n".join(lines) + "\n")
