"""Curve skeletons on both routes at the size of a kidney CT: a synthetic 512x512x256 volume holding a branching vessel
tree (three generations of tubes whose radius shrinks from 5 to 2 voxels) and a kidney-sized ellipsoid, thinned once by
the numpy twin on the host (transform._skeleton_numpy - it takes minutes) and by csrc/skeleton.hip on the device
(skeleton.thin on a packed mask that already lives in HBM; median of REPS passes after a warm-up pass, timed between
synchronises).  The two skeletons are asserted equal voxel for voxel before anything is printed.  Then the measures on
the skeleton (classify, length, radii) on both routes, asserted equal.  Prints iterations, kernel launches and one line
per stage, a JSON summary line, and writes the same text to profiles/skeleton_512x512x256_host_vs_device.txt.
`--device-only` skips the host route and the comparisons: the run to put under `rocprofv3 --kernel-trace --stats`."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "3d-unet-renal-anatomy-extraction_amd"))
import numpy as np, torch, morphology, skeleton, trainer, transform
dev = torch.device("cuda:0")
SHAPE, SPACING, REPS = (512, 512, 256), (0.75, 0.75, 3.0), 7
DEVICE_ONLY = "--device-only" in sys.argv
OUT = os.path.join(ROOT, "profiles", "skeleton_%dx%dx%d_host_vs_device.txt" % SHAPE)


def tube(volume, a, b, radius):
    """Set the voxels within `radius` of the segment a - b."""
    a, b = np.asarray(a, float), np.asarray(b, float)
    lo = np.maximum(np.floor(np.minimum(a, b) - radius).astype(int), 0)
    hi = np.minimum(np.ceil(np.maximum(a, b) + radius).astype(int) + 1, volume.shape)
    p = np.stack(np.meshgrid(*[np.arange(l, h) for l, h in zip(lo, hi)], indexing="ij"), axis=-1).astype(float)
    t = np.clip(((p - a) * (b - a)).sum(-1) / ((b - a) ** 2).sum(), 0, 1)
    d2 = ((p - (a + t[..., None] * (b - a))) ** 2).sum(-1)
    volume[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] |= d2 <= radius * radius


def grow(volume, start, direction, length, radius, depth, rng):
    end = start + direction * length
    tube(volume, start, end, radius)
    if depth:
        for sign in (-1, 1):
            turn = np.cross(direction, rng.randn(3))
            turn /= np.linalg.norm(turn)
            d = direction + 0.9 * sign * turn
            grow(volume, end, d / np.linalg.norm(d), length * 0.7, max(radius * 0.7, 2.0), depth - 1, rng)


rng = np.random.RandomState(0)
volume = np.zeros(SHAPE, bool)
grow(volume, np.array([60.0, 256.0, 128.0]), np.array([1.0, 0.0, 0.0]), 120.0, 5.0, 3, rng)
x, y, z = np.ogrid[:SHAPE[0], :SHAPE[1], :SHAPE[2]]
volume |= ((x - 400) / 70.0) ** 2 + ((y - 120) / 90.0) ** 2 + ((z - 128) / 55.0) ** 2 < 1        # the kidney-sized blob
lines = []


def say(text):
    print(text); lines.append(text)


def timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter(); out = fn(); torch.cuda.synchronize()
    return out, 1e3 * (time.perf_counter() - t0)


host_ms = {}
if not DEVICE_ONLY:
    t0 = time.perf_counter(); h_skel, h_iterations = transform._skeleton_numpy(volume); host_ms["thin"] = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter(); h_class = transform._skeleton_classify_numpy(h_skel)[2:]; host_ms["classify"] = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter(); h_length = transform._skeleton_length_numpy(h_skel, SPACING); host_ms["length"] = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    h_radii = trainer._radius_stats_numpy(trainer._radii_squared_numpy(h_skel, volume, SPACING))[1:]
    host_ms["radii"] = 1e3 * (time.perf_counter() - t0)

mask = morphology.pack(torch.from_numpy(volume).to(dev))
passes = {"thin": [], "classify": [], "length": [], "radii": []}
for rep in range(REPS + 1):                                                  # pass 0 warms up: code objects, allocator, workspace
    (d_skel, d_iterations), ms = timed(lambda: skeleton.thin(mask, return_iterations=True)); passes["thin"].append(ms)
    d_class, ms = timed(lambda: skeleton.classify(d_skel)[2:]); passes["classify"].append(ms)
    d_length, ms = timed(lambda: skeleton.length(d_skel, SPACING)); passes["length"].append(ms)
    d_radii, ms = timed(lambda: skeleton.radii(d_skel, mask, SPACING)); passes["radii"].append(ms)
dev_ms = {stage: float(np.median(v[1:])) for stage, v in passes.items()}
if not DEVICE_ONLY:
    assert d_iterations == h_iterations
    assert (morphology.unpack(d_skel).cpu().numpy().astype(bool) == h_skel).all()
    assert d_class == h_class and d_length == h_length and d_radii == h_radii, (d_class, h_class, d_length, h_length, d_radii, h_radii)

subfields = sum(1 for s in range(8) if (s >> 2) < SHAPE[0] and ((s >> 1) & 1) < SHAPE[1] and (s & 1) < SHAPE[2])
say("volume %s, spacing %s: %d object voxels -> %d skeleton voxels, %d ends, %d junction voxels" % (
    (SHAPE, SPACING, int(volume.sum())) + tuple(d_class)))
say("graph length %.1f mm, radius min / mean / max %.2f / %.2f / %.2f mm" % ((d_length,) + tuple(d_radii)))
say("thinning: %d iterations (the last one idle), %d kernel launches (%d per iteration: 6 candidate markings, %d sub-passes), "
    "%d host reads" % (d_iterations, d_iterations * 6 * (1 + subfields), 6 * (1 + subfields), 6 * subfields, d_iterations))
if not DEVICE_ONLY:
    say("host route (once; the numpy twin, scipy for the radii)")
    for stage, ms in host_ms.items():
        say("  %-12s %12.1f ms" % (stage, ms))
say("device route (median of %d passes after a warm-up pass)" % REPS)
for stage, ms in dev_ms.items():
    say("  %-12s %12.3f ms" % (stage, ms))
say(json.dumps({"shape": SHAPE, "spacing": SPACING, "reps": REPS, "iterations": d_iterations,
                "host_ms": {s: round(v, 1) for s, v in host_ms.items()}, "device_ms": {s: round(v, 3) for s, v in dev_ms.items()},
                "identical_outputs": not DEVICE_ONLY or None}))
if not DEVICE_ONLY:
    out = os.environ.get("RU3D_OUT")
    path = os.path.join(out, os.path.basename(OUT)) if out else OUT
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
