"""What the plain 3D U-Net (ConvBlockStack / MaxPoolBlock, the assembler's own defaults) costs on the native path.
(a) The pooling kernel at 2 x 64 x 128^3 bf16: ru3d_maxpool3d_fwd / _bwd against torch.nn.functional.max_pool3d forward /
    backward on the same channels_last_3d tensor (the route before the kernel existed) and against ru3d_add on the same
    tensor in the same run (the project's own streaming yardstick), with the achieved bytes/s of the byte model:
    forward x + y + idx, backward dy + idx + dx, add 3 x.
(b) The training step of Unet(1, 3, generate_paired_features2(4, 32)) at 2 x SIZE^3 (SIZE = 128, or argv[1]), HybirdLoss,
    optim.Adam: bf16 storage on the native blocks, captured (graph.GraphedTrainStep) and eager, and the launch names of
    one native forward per block; unless `--native-only` is given, also the same model with RU3D_PLAIN_BLOCKS=torch - the
    blocks as torch modules in fp32 storage, which is what this model ran as before (eager: torch's conv library is not
    captured here).  At 2 x 128^3 torch's conv library spends minutes choosing its fp32 kernels before the first step
    returns: time that route at SIZE = 64.
Timing: WARM warm-up passes, then ROUNDS rounds that alternate between the candidates; a round times REPS passes of one
candidate between two HIP events and takes their mean; the figure is the median over the rounds, the spread is (max - min)
over the rounds.  Prints one line per figure and a JSON summary line, and writes the same text to
profiles/plain_unet_2x128.txt (or $RU3D_OUT)."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "3d-unet-renal-anatomy-extraction_amd"))
import numpy as np, torch, torch.nn.functional as F
import _native as N, _ops as ops, graph, loss as L, network, optim
from oracle import unet_oracle as O
dev = torch.device("cuda:0")
ARGS = [a for a in sys.argv[1:] if not a.startswith("--")]
SIZE = int(ARGS[0]) if ARGS else 128
NATIVE_ONLY = "--native-only" in sys.argv
WARM, ROUNDS, REPS, STEP_REPS = 3, 7, 20, 3
OUT = os.path.join(ROOT, "profiles", "plain_unet_2x128.txt")
lines = []


def say(text):
    print(text, flush=True); lines.append(text)


def alternate(candidates, reps, warm=WARM, rounds=ROUNDS):
    """{name: (median ms per pass, spread ms)} of callables timed in alternating rounds."""
    for k, fn in candidates.items():
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        print("  (warmed up: %s)" % k, flush=True)
    torch.cuda.synchronize()
    got = {k: [] for k in candidates}
    for _ in range(rounds):
        for k, fn in candidates.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record(); b.synchronize()
            got[k].append(a.elapsed_time(b) / reps)
    return {k: (float(np.median(v)), float(max(v) - min(v))) for k, v in got.items()}


# ------------------------------------------------------------------------------------------- (a) the pooling kernel
n, c, s = 2, 64, 128
x = torch.empty((n, s, s, s, c), dtype=torch.bfloat16, device=dev).normal_().permute(0, 4, 1, 2, 3)
x2 = torch.empty_like(x).normal_()
y, idx = ops.maxpool_fwd(x)
gy = torch.empty_like(y).normal_()
xt = x.detach().clone().requires_grad_(True)          # channels_last_3d strides survive the clone
yt = F.max_pool3d(xt, 2, 2)
assert torch.equal(yt.detach(), y), "the kernel and torch disagree on the pooled values"
xb, yb, ib = x.numel() * 2, y.numel() * 2, idx.numel()
models = {"ru3d_maxpool3d_fwd": xb + yb + ib, "ru3d_maxpool3d_bwd": yb + ib + xb, "ru3d_add": 3 * xb}
pool_ms = alternate({
    "ru3d_maxpool3d_fwd": lambda: ops.maxpool_fwd(x),
    "torch max_pool3d fwd": lambda: F.max_pool3d(x, 2, 2),
    "ru3d_maxpool3d_bwd": lambda: ops.maxpool_bwd(gy, idx, tuple(x.shape)),
    "torch max_pool3d bwd": lambda: torch.autograd.grad(yt, xt, gy, retain_graph=True),
    "ru3d_add": lambda: ops.add(x, x2)}, REPS)
say("pooling at %s bf16 NDHWC; HIP-event times per call: median of %d alternating rounds of %d calls, %d warm-up calls; "
    "spread = max - min over the rounds" % ((n, c, s, s, s), ROUNDS, REPS, WARM))
for k, (t, sp) in pool_ms.items():
    rate = "   %6.2f TB/s of %4d MB" % (models[k] / t / 1e9, models[k] // (1 << 20)) if k in models else ""
    say("  %-24s %8.4f ms   (spread %.4f)%s" % (k, t, sp, rate))
rate = {k: models[k] / pool_ms[k][0] for k in models}
say("  byte rate against ru3d_add: forward %.2f, backward %.2f; time against torch: forward %.2f x, backward %.2f x" % (
    rate["ru3d_maxpool3d_fwd"] / rate["ru3d_add"], rate["ru3d_maxpool3d_bwd"] / rate["ru3d_add"],
    pool_ms["torch max_pool3d fwd"][0] / pool_ms["ru3d_maxpool3d_fwd"][0],
    pool_ms["torch max_pool3d bwd"][0] / pool_ms["ru3d_maxpool3d_bwd"][0]))
del x, x2, y, idx, gy, xt, yt
torch.cuda.empty_cache()

# ------------------------------------------------------------------------------------------- (b) the training step
shape = (2, 1, SIZE, SIZE, SIZE)
xin = O.synth_image(shape, 1).to(dev)
lab = O.phantom_labels(2, shape[2:], 3).to(dev)


def make(dtype):
    torch.manual_seed(0)
    model = network.Unet(1, 3, network.generate_paired_features2(4, 32)).to(dev)
    network.set_compute_dtype(model, dtype)
    model.train()
    return model, optim.Adam(model.parameters(), lr=1e-4), L.HybirdLoss()


def eager_step(model, opt, crit):
    def run():
        opt.zero_grad(set_to_none=True)
        crit(model(xin), lab).backward()
        opt.step()
    return run


def torch_blocks(fn):
    def run():
        os.environ["RU3D_PLAIN_BLOCKS"] = "torch"
        try:
            fn()
        finally:
            os.environ.pop("RU3D_PLAIN_BLOCKS", None)
    return run


model, opt, crit = make(torch.bfloat16)
assert model._native_chain() is not None and model._storage_dtype() == torch.bfloat16
names = {}
hooks = []
order = []


def note(tag):
    order.append(tag)
    names[tag] = N.lib.ru3d_launch_log_end().decode()


for kind, blocks in (("encode", model.encode_blocks), ("pool", model.pool_blocks), ("up", model.up_blocks),
                     ("decode", model.decode_blocks)):
    for i, blk in enumerate(blocks):
        tag = "%s %d" % (kind, i)
        hooks.append(blk.register_forward_pre_hook(lambda m, a: N.lib.ru3d_launch_log_begin()))
        hooks.append(blk.register_forward_hook(lambda m, a, o, tag=tag: note(tag)))
model(xin)
for h in hooks:
    h.remove()
say("plain Unet(1, 3, generate_paired_features2(4, 32)), batch %s, HybirdLoss, optim.Adam" % (shape,))
say("launches of one native bf16 forward, per block in execution order:")
for tag in order:
    say("  %-9s %s" % (tag, names[tag]))
graphed = graph.GraphedTrainStep(model, crit, opt, warmup=2)
model_e, opt_e, crit_e = make(torch.bfloat16)
candidates = {"native blocks, bf16, graph replay": lambda: graphed(xin, lab),
              "native blocks, bf16, eager": eager_step(model_e, opt_e, crit_e)}
if not NATIVE_ONLY:
    model_t, opt_t, crit_t = make(torch.bfloat16)
    candidates["torch blocks, fp32 storage, eager"] = torch_blocks(eager_step(model_t, opt_t, crit_t))
step_ms = alternate(candidates, STEP_REPS, warm=3, rounds=5)
L.raise_on_bad_labels(wait=True)
assert graphed.replays > 0
for k, (t, sp) in step_ms.items():
    say("  %-36s %9.3f ms   (spread %.3f)" % (k, t, sp))
if not NATIVE_ONLY:
    a, b, t = (step_ms[k][0] for k in step_ms)
    say("  torch blocks / native replay %.2f x, torch blocks / native eager %.2f x" % (t / a, t / b))
say(json.dumps({"pool_shape": (n, c, s, s, s), "step_shape": shape, "rounds": ROUNDS, "reps": REPS, "step_reps": STEP_REPS,
                "pool_ms": {k: [round(v, 4), round(sp, 4)] for k, (v, sp) in pool_ms.items()},
                "pool_bytes": models,
                "step_ms": {k: [round(v, 3), round(sp, 3)] for k, (v, sp) in step_ms.items()}}))
graphed.release()
out = os.environ.get("RU3D_OUT")
name = os.path.basename(OUT) if SIZE == 128 else "plain_unet_2x%d.txt" % SIZE
path = os.path.join(out, name) if out else os.path.join(os.path.dirname(OUT), name)
with open(path, "w") as fh:
    fh.write("\n".join(lines) + "\n")
