"""Per-stage times of the surface-distance metrics of one prediction on both routes: the synthetic 512x512x256
three-class prediction of tools/post_bench.py against its shifted label through trainer.evaluate_surface_case, once with
scipy / numpy on the host and once with csrc/distance.hip on the device, where the prediction and the label already
live in HBM.  Stages (summed over the three classes): surfaces (class mask and mask & ~erosion, twice per class),
transform (two per class: scipy's feature transform / the squared distance transform), gather (the squared distances
at the other surface's voxels), reductions (maxima, tolerance counts, order statistics, sums of roots; on the device
including the one download of ten numbers).  Device stages are timed between synchronises after a warm-up pass, median
of REPS passes; the host route runs once (it takes minutes).  The two routes' statistics are asserted equal before
anything is printed.  The adversarial case of the outward scan follows: one feature voxel in a corner, where every
voxel scans until it meets that corner's row, against scipy.ndimage.distance_transform_edt of the same volume.
Prints one line per stage and a JSON summary line.  `--device-only` skips the host route and the comparisons: the run
to put under `rocprofv3 --kernel-trace --stats` (tools/kstats.py summarises it)."""
import json, math, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "3d-unet-renal-anatomy-extraction_amd"))
import numpy as np, scipy.ndimage as ndi, torch, distance, morphology, trainer
dev = torch.device("cuda:0")
SHAPE, SPACING, TOLERANCE, REPS, CLASSES = (512, 512, 256), (0.75, 0.75, 3.0), 1.5, 7, 3
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
times = {"host": {}, "device": {}}


def host(stage, fn):
    t0 = time.perf_counter(); out = fn()
    times["host"][stage] = times["host"].get(stage, 0.0) + 1e3 * (time.perf_counter() - t0)
    return out


def device(stage, fn):
    torch.cuda.synchronize(); t0 = time.perf_counter(); out = fn(); torch.cuda.synchronize()
    passes = times["device"].setdefault(stage, [0.0])
    passes[-1] += 1e3 * (time.perf_counter() - t0)
    return out


# ---- host route: the stages of trainer._surface_stats_numpy, class by class
h_stats = []
for c in range(1, CLASSES + 1):
    if DEVICE_ONLY:
        break
    sa, sb = host("surfaces", lambda: (trainer._surface_numpy(pred == c), trainer._surface_numpy(label == c)))
    near_b, near_a = host("transform", lambda: (trainer._nearest_feature_numpy(sb, SPACING),
                                                trainer._nearest_feature_numpy(sa, SPACING)))
    d_ab, d_ba = host("gather", lambda: (trainer._contract_sq_numpy(sa, near_b, SPACING),
                                         trainer._contract_sq_numpy(sb, near_a, SPACING)))
    h_stats.append(host("reductions", lambda: trainer._surface_reduce_numpy(d_ab, d_ba, TOLERANCE)))
    del near_a, near_b

# ---- device route: the stages of distance.surface_stats, class by class
d_pred, d_label = torch.from_numpy(pred).to(dev), torch.from_numpy(label).to(dev)
cap = distance._INITIAL_CAPACITY


def device_reductions(both, counts):
    red = [distance.reduce(both[:cap], counts[0:1], TOLERANCE * TOLERANCE), distance.reduce(both[cap:], counts[1:2], TOLERANCE * TOLERANCE)]
    ordered = torch.sort(both).values
    n = counts.sum()
    lo = torch.floor((n - 1).to(torch.float64) * 0.95).to(torch.int64)
    return torch.cat((counts.to(torch.float64), red[0][1:], red[1][1:], ordered[torch.stack((lo, lo + 1))])).cpu().numpy()


for rep in range(REPS + 1):                                                  # pass 0 warms up: code objects, allocator, workspace
    if rep == 1:
        times["device"] = {}
    for passes in times["device"].values():
        passes.append(0.0)
    d_stats = []
    for c in range(1, CLASSES + 1):
        sa, sb = device("surfaces", lambda: (distance.surface(morphology.pack(d_pred, "eq", c)),
                                             distance.surface(morphology.pack(d_label, "eq", c))))
        to_b, to_a = device("transform", lambda: (distance.edt_squared(sb, SPACING), distance.edt_squared(sa, SPACING)))
        both = torch.full((2 * cap,), float("inf"), dtype=torch.float64, device=dev)
        counts = torch.empty(2, dtype=torch.int64, device=dev)
        device("gather", lambda: (distance._gather_into(to_b, sa, both[:cap], counts[0:1]),
                                  distance._gather_into(to_a, sb, both[cap:], counts[1:2])))
        got = device("reductions", lambda: device_reductions(both, counts))
        d_stats.append(dict(n_ab=int(got[0]), n_ba=int(got[1]), max_ab=got[2], within_ab=int(got[3]), sum_ab=got[4],
                            max_ba=got[5], within_ba=int(got[6]), sum_ba=got[7], lo=got[8], hi=got[9]))
        del to_a, to_b
    d_metrics = device("evaluate_surface_case (whole call)", lambda: trainer.evaluate_surface_case(
        {"pred": d_pred, "label": d_label}, spacing=SPACING, tolerance=TOLERANCE))
dev_ms = {s: float(np.median(v)) for s, v in times["device"].items()}
assert all(max(s["n_ab"], s["n_ba"]) <= cap for s in d_stats)
staged = [trainer._surface_metrics(s) for s in d_stats]
assert all(m[k] == w[k] for m, w in zip(d_metrics, staged) for k in ("hd", "hd95", "assd", "nsd"))
if not DEVICE_ONLY:
    for h, d in zip(h_stats, d_stats):
        assert all(h[k] == d[k] for k in h if not k.startswith("sum")), (h, d)
        assert all(math.isclose(h[k], d[k], rel_tol=1e-12) for k in ("sum_ab", "sum_ba")), (h, d)

# ---- the adversarial case: one feature voxel in a corner
corner = np.zeros(SHAPE, bool)
corner[0, 0, 0] = True
d_corner = morphology.pack(torch.from_numpy(corner).to(dev))
corner_ms = []
for rep in range(REPS + 1):
    torch.cuda.synchronize(); t0 = time.perf_counter(); d_far = distance.edt_squared(d_corner, SPACING); torch.cuda.synchronize()
    corner_ms.append(1e3 * (time.perf_counter() - t0))
dev_ms["transform, one feature in a corner"] = float(np.median(corner_ms[1:]))
far = d_far.cpu().numpy()
assert np.array_equal(far, (SPACING[0] * x.astype(np.float64)) ** 2 + ((SPACING[1] * y.astype(np.float64)) ** 2
                                                                       + (SPACING[2] * z.astype(np.float64)) ** 2))
if not DEVICE_ONLY:
    h_far = host("transform, one feature in a corner", lambda: ndi.distance_transform_edt(~corner, sampling=SPACING))
    assert np.array_equal(np.sqrt(far), h_far)

print("volume %s, spacing %s, tolerance %s; surface voxels (pred, label) per class %s" % (
    SHAPE, SPACING, TOLERANCE, [(s["n_ab"], s["n_ba"]) for s in d_stats]))
print("metrics per class: %s" % [{k: round(v, 6) for k, v in m.items()} for m in d_metrics])
if not DEVICE_ONLY:
    print("host route (once; scipy.ndimage + numpy, summed over the %d classes)" % CLASSES)
for stage, ms in times["host"].items():
    print("  %-40s %10.1f ms" % (stage, ms))
print("device route (median of %d passes after a warm-up pass, summed over the %d classes)" % (REPS, CLASSES))
for stage, ms in dev_ms.items():
    print("  %-40s %10.3f ms" % (stage, ms))
print(json.dumps({"shape": SHAPE, "spacing": SPACING, "reps": REPS, "host_ms": {s: round(v, 1) for s, v in times["host"].items()},
                  "device_ms": {s: round(v, 3) for s, v in dev_ms.items()}, "identical_outputs": not DEVICE_ONLY or None}))
