"""Per-stage times of the clean-up and the evaluation of one prediction on both routes: a synthetic 512x512x256
three-class mask (two organ-sized blobs of class 1 with class 2 and class 3 inside, pin holes in class 2, 0.1 % speckle)
through transform.post_transform and trainer.evaluate_case / evaluate_metrics, once with scipy / numpy on the host and
once with csrc/morphology.hip + csrc/components.hip on the device, where the prediction and the label already live in
HBM (the cascade left them there).  Device stages are timed between synchronises after a warm-up pass, median of REPS
passes; the host route runs once (it takes seconds).  The two routes' outputs are asserted equal before anything is
printed.  Prints one line per stage and a JSON summary line.  `--device-only` skips the host route and the comparison:
the run to put under `rocprofv3 --kernel-trace --stats` (tools/kstats.py summarises it)."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "3d-unet-renal-anatomy-extraction_amd"))
import numpy as np, scipy.ndimage as ndi, torch, components, morphology, trainer, transform
dev = torch.device("cuda:0")
SHAPE, THRESHOLD, LABEL, REPS = (512, 512, 256), 10000, 2, 7
DEVICE_ONLY = "--device-only" in sys.argv
rng = np.random.RandomState(0)
x, y, z = np.ogrid[:SHAPE[0], :SHAPE[1], :SHAPE[2]]


def blob(c, r):
    return ((x - c[0]) / float(r[0])) ** 2 + ((y - c[1]) / float(r[1])) ** 2 + ((z - c[2]) / float(r[2])) ** 2 < 1


pred = np.zeros(SHAPE, np.uint8)
for c in ((150, 260, 120), (380, 250, 130)):
    pred[blob(c, (90, 115, 72))] = 1
    pred[blob(c, (55, 70, 45))] = 2
    pred[blob((c[0] + 10, c[1], c[2]), (20, 25, 15))] = 3
pred[(pred == 2) & (rng.rand(*SHAPE) < 0.01)] = 1
speckle = rng.rand(*SHAPE) < 0.001
pred[speckle] = rng.randint(1, 4, size=int(speckle.sum())).astype(np.uint8)
label = np.roll(pred, (3, -2, 1), axis=(0, 1, 2))
ball = transform.create_sphere((7, 7, 7), (3, 3, 3), 4)
times = {"host": {}, "device": {}}


def host(stage, fn):
    t0 = time.perf_counter(); out = fn()
    times["host"][stage] = 1e3 * (time.perf_counter() - t0)
    return out


def device(stage, fn):
    torch.cuda.synchronize(); t0 = time.perf_counter(); out = fn(); torch.cuda.synchronize()
    times["device"].setdefault(stage, []).append(1e3 * (time.perf_counter() - t0))
    return out


# ---- host route: the stages of transform.post_transform's numpy branch, then the evaluation
h_out = np.zeros_like(pred)
h_fg = DEVICE_ONLY or host("foreground + small-region filter", lambda: transform.remove_small_region(pred > 0, THRESHOLD))
h_closed = DEVICE_ONLY or host("closing (7^3 ball)", lambda: ndi.binary_closing(pred == LABEL, ball))
h_kd = DEVICE_ONLY or host("opening (cross)", lambda: ndi.binary_opening(h_closed))


def host_compose():
    h_out[h_fg] = 1; h_out[h_kd] = LABEL
    return h_out


if not DEVICE_ONLY:
    host("compose output", host_compose)
    h_total = host("post_transform (whole call)", lambda: transform.post_transform(pred))
    assert np.array_equal(h_total, h_out)
    h_dice = host("evaluate_case", lambda: trainer.evaluate_case({"pred": h_out, "label": label}))
    h_metrics = host("evaluate_metrics", lambda: trainer.evaluate_metrics({"pred": h_out, "label": label}))

# ---- device route: the same stages as transform.post_transform's HIP branch runs them
d_pred, d_label = torch.from_numpy(pred).to(dev), torch.from_numpy(label).to(dev)
for rep in range(REPS + 1):                                                  # pass 0 warms up: code objects, allocator, workspace
    if rep == 1:
        times["device"] = {}
    d_fgbits = device("pack (pred > 0)", lambda: morphology.pack(d_pred, "gt", 0))
    d_out = device("unpack foreground bytes", lambda: morphology.unpack(d_fgbits, 1))
    device("label + stats + filter", lambda: components.remove_small_region(d_out, THRESHOLD))
    d_kdbits = device("pack (pred == 2)", lambda: morphology.pack(d_pred, "eq", LABEL))
    d_closed = device("closing (7^3 ball)", lambda: morphology.close(d_kdbits, ball))
    d_kd = device("opening (cross)", lambda: morphology.open(d_closed))
    device("paint label into output", lambda: morphology.unpack(d_kd, LABEL, out=d_out, paint=True))
    d_total = device("post_transform (whole call)", lambda: transform.post_transform(d_pred))
    d_dice = device("evaluate_case", lambda: trainer.evaluate_case({"pred": d_total, "label": d_label}))
    d_metrics = device("evaluate_metrics", lambda: trainer.evaluate_metrics({"pred": d_total, "label": d_label}))
dev_ms = {s: float(np.median(v)) for s, v in times["device"].items()}

assert torch.equal(d_out, d_total) and np.array_equal(d_pred.cpu().numpy(), pred)
if not DEVICE_ONLY:
    assert np.array_equal(d_total.cpu().numpy(), h_out)
    assert np.allclose(d_dice, h_dice, rtol=0, atol=1e-6) and d_metrics == h_metrics
print("volume %s, %d voxels differ between post_transform's output and its input, dice %s" % (
    SHAPE, int((d_total.cpu().numpy() != pred).sum()), ["%.6f" % v for v in d_dice]))
if not DEVICE_ONLY:
    print("host route (once)")
for stage, ms in times["host"].items():
    print("  %-36s %10.1f ms" % (stage, ms))
print("device route (median of %d passes after a warm-up pass; evaluate_* include the download of the 33 x 33 table)" % REPS)
for stage, ms in dev_ms.items():
    print("  %-36s %10.3f ms" % (stage, ms))
print(json.dumps({"shape": SHAPE, "reps": REPS, "host_ms": {s: round(v, 1) for s, v in times["host"].items()},
                  "device_ms": {s: round(v, 3) for s, v in dev_ms.items()}, "identical_outputs": not DEVICE_ONLY or None}))
