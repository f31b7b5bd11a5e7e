"""Times of the prediction clean-up on one seeded synthetic prediction at 512x512x256: two ellipsoid kidneys (1) with
background cavities, a tumour (2) enclosed in one of them, and spurious specks.

fill_holes of `pred == 1`, three routes:
  host      scipy.ndimage.binary_fill_holes on the numpy volume (once)
  composed  what the device could do before csrc/propagate.hip: components.label of the complement, components.stats,
            one download of the boxes, and every component whose box touches no face of the volume painted into the mask
  flood     transform.binary_fill_holes: pack, the rounds of csrc/propagate.hip, unpack
keep_largest of `pred > 0`, k = 2: the numpy route (once) against transform.keep_largest_region on the device.

The device routes are timed with device events in one run after a warm-up pass, alternating the routes inside every
pass, median of REPS passes; the three results of fill_holes are asserted equal voxel for voxel, and so are the two of
keep_largest, before anything is printed.  Prints one line per route, the rounds the flood took, and one JSON line.
`--shape X Y Z` times another size; `--device-only` skips the host routes and their comparisons."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "3d-unet-renal-anatomy-extraction_amd"))
import numpy as np, scipy.ndimage as ndi, torch
import components, morphology, transform
if not torch.cuda.is_available():
    sys.exit("postprocess_bench: no HIP device (a time taken without one says nothing about the kernels)")
dev = torch.device("cuda:0")
REPS = 7
SHAPE = tuple(int(v) for v in sys.argv[sys.argv.index("--shape") + 1:sys.argv.index("--shape") + 4]) if "--shape" in sys.argv \
    else (512, 512, 256)
DEVICE_ONLY = "--device-only" in sys.argv


def phantom(shape, seed=0):
    rng = np.random.RandomState(seed)
    x, y, z = np.ogrid[:shape[0], :shape[1], :shape[2]]

    def blob(c, r):
        return ((x - c[0]) / r[0]) ** 2 + ((y - c[1]) / r[1]) ** 2 + ((z - c[2]) / r[2]) ** 2 < 1

    s = np.array(shape, dtype=np.float64)
    v = np.zeros(shape, np.uint8)
    v[blob(s * (0.3, 0.5, 0.5), s * (0.09, 0.07, 0.2))] = 1
    v[blob(s * (0.7, 0.5, 0.45), s * (0.085, 0.07, 0.19))] = 1
    v[blob(s * (0.3, 0.5, 0.5), s * (0.03, 0.03, 0.07))] = 2                    # enclosed in the first kidney
    for _ in range(12):                                                        # cavities well inside the kidneys
        k = rng.randint(2)
        c = s * ((0.3, 0.5, 0.5), (0.7, 0.5, 0.45))[k] + rng.uniform(-1, 1, 3) * s * (0.04, 0.03, 0.1)
        hole = blob(c, s * 0.004 * rng.uniform(1, 3, 3) + 1)
        v[hole & (v == 1)] = 0
    for _ in range(200):                                                       # specks
        c = (rng.uniform(0.02, 0.98, 3) * s).astype(int)
        e = rng.randint(1, 4, 3)
        v[c[0]:c[0] + e[0], c[1]:c[1] + e[1], c[2]:c[2] + e[2]] = 1 + rng.randint(2)
    return v


def composed_fill(mask_bytes):
    """binary_fill_holes from the labelling of the complement: the components whose box touches no face are holes."""
    complement = (mask_bytes == 0).to(torch.uint8)
    labels, count = components.label(complement)
    _, boxes = components.stats(labels, count)
    b = boxes.cpu().numpy()
    X, Y, Z = labels.shape
    inner = (b[:, 0] > 0) & (b[:, 1] < X) & (b[:, 2] > 0) & (b[:, 3] < Y) & (b[:, 4] > 0) & (b[:, 5] < Z)
    table = torch.from_numpy(np.concatenate([[False], inner])).to(labels.device)
    return (mask_bytes != 0) | table[labels.long()]


def flood_fill(mask_bytes):
    return transform.binary_fill_holes(mask_bytes)


def keep_two(foreground):
    return transform.keep_largest_region(foreground, 2)


def timed(fn, *args):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record(); out = fn(*args); stop.record(); torch.cuda.synchronize()
    return start.elapsed_time(stop), out


pred = phantom(SHAPE)
volume = torch.from_numpy(pred).to(dev)
kidney = (volume == 1).to(torch.uint8)
foreground = (volume != 0).to(torch.uint8)
routes = {"fill_holes: composed (label the complement)": (composed_fill, lambda: (kidney,)),
          "fill_holes: flood": (flood_fill, lambda: (kidney,)),
          "keep_largest k=2: device": (keep_two, lambda: (foreground.clone(),))}
for fn, args in routes.values():                                              # warm-up: code objects, allocator, workspace
    fn(*args())
torch.cuda.synchronize()
times, got = {name: [] for name in routes}, {}
for _ in range(REPS):
    for name, (fn, args) in routes.items():                                    # the routes alternate inside every pass
        ms, got[name] = timed(fn, *args())
        times[name].append(ms)
flood_fill(kidney)
rounds = morphology.last_rounds
dev_ms = {name: float(np.median(v)) for name, v in times.items()}
spread = {name: (float(min(v)), float(max(v))) for name, v in times.items()}
assert torch.equal(got["fill_holes: composed (label the complement)"], got["fill_holes: flood"])
holes = int(got["fill_holes: flood"].sum()) - int(kidney.sum())
host_ms = {}
if not DEVICE_ONLY:
    t0 = time.perf_counter(); want = ndi.binary_fill_holes(pred == 1)
    t1 = time.perf_counter(); kept = transform.keep_largest_region(pred > 0, 2)
    t2 = time.perf_counter()
    host_ms = {"fill_holes: host (scipy)": 1e3 * (t1 - t0), "keep_largest k=2: host (scipy label + numpy)": 1e3 * (t2 - t1)}
    assert np.array_equal(got["fill_holes: flood"].cpu().numpy(), want)
    assert np.array_equal(got["keep_largest k=2: device"].cpu().numpy() != 0, kept)
print("prediction %s uint8: %d voxels of class 1 with %d hole voxels (%d of them the enclosed tumour), %d foreground "
      "components" % (SHAPE, int(kidney.sum()), holes, int(((volume == 2) & got["fill_holes: flood"]).sum()),
                      components.label(foreground)[1]))
if not DEVICE_ONLY:
    print("host routes (once)")
    for name, ms in host_ms.items():
        print("  %-50s %10.1f ms" % (name, ms))
print("device routes (device events, median of %d alternating passes after a warm-up pass; min .. max)" % REPS)
for name, ms in dev_ms.items():
    print("  %-50s %10.3f ms   %8.3f .. %.3f" % (name, ms, spread[name][0], spread[name][1]))
print("the flood ran %d rounds (batches of 8, 16, 32, 64 with one read-back each; the last batch's overshoot included)" % rounds)
print(json.dumps({"shape": SHAPE, "reps": REPS, "hole_voxels": holes, "flood_rounds": rounds,
                  "host_ms": {s: round(v, 1) for s, v in host_ms.items()},
                  "device_ms": {s: round(v, 3) for s, v in dev_ms.items()},
                  "identical_outputs": True}))
