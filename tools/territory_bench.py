"""Vessel territories at the size of a kidney CT: a synthetic 512x512x256 label volume (a kidney-sized ellipsoid, label 2; a
branching arterial tree of three generations inside it, label 1; a spherical tumour, label 3) on the device route of
territory.nearest, territory.assign + territory.tally and the whole driver trainer.vessel_territories_case, with
distance.edt_squared timed on the same site mask for comparison (the feature transform moves 12 bytes per voxel and pass
where edt_squared moves 8).  Device times are medians of REPS passes after a warm-up pass, each pass timed between
synchronises straight after an untimed call that keeps the clocks up.  On the host, at the full size: scipy's feature
transform (what a host user has; the numpy twin of `nearest` is a definition that visits every candidate of a row and is
not run at this size) and the assign and tally twins, which are asserted equal to the device.  The twins of `nearest` and
of the whole driver run on the same scene at a quarter of the resolution (--check-shape), where both routes are timed and
asserted equal.  Prints one line per stage and a JSON summary line, and writes the same text to
profiles/territories_512x512x256.txt.  `--host-only` builds the scenes and runs the host parts alone."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "3d-unet-renal-anatomy-extraction_amd"))
import numpy as np, scipy.ndimage as ndi, torch
import territory, trainer, transform

ap = argparse.ArgumentParser()
ap.add_argument("--shape", type=int, nargs=3, default=(512, 512, 256))
ap.add_argument("--check-shape", type=int, nargs=3, default=(128, 128, 64))
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--host-only", action="store_true")
args = ap.parse_args()
SHAPE, CHECK, REPS = tuple(args.shape), tuple(args.check_shape), args.reps
OUT = os.path.join(ROOT, "profiles", "territories_%dx%dx%d.txt" % SHAPE)
lines = []


def say(text):
    print(text, flush=True); lines.append(text)


def tube(volume, a, b, radius):
    """Set the voxels within `radius` of the segment a - b."""
    lo = np.maximum(np.floor(np.minimum(a, b) - radius).astype(int), 0)
    hi = np.minimum(np.ceil(np.maximum(a, b) + radius).astype(int) + 1, volume.shape)
    p = np.stack(np.meshgrid(*[np.arange(l, h) for l, h in zip(lo, hi)], indexing="ij"), axis=-1).astype(float)
    t = np.clip(((p - a) * (b - a)).sum(-1) / ((b - a) ** 2).sum(), 0, 1)
    volume[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] |= ((p - (a + t[..., None] * (b - a))) ** 2).sum(-1) <= radius * radius


def grow(volume, start, direction, length, radius, depth, rng):
    end = start + direction * length
    tube(volume, start, end, radius)
    if depth:
        for sign in (-1, 1):
            turn = np.cross(direction, rng.randn(3))
            d = direction + 0.9 * sign * turn / np.linalg.norm(turn)
            grow(volume, end, d / np.linalg.norm(d), length * 0.7, max(radius * 0.7, 1.5), depth - 1, rng)


def scene(shape):
    """uint8 label volume of `shape`: kidney 2, arterial tree 1, tumour 3; every length scales with the shape."""
    s = np.array(shape, float) / (512.0, 512.0, 256.0)
    k = float(s.min())
    x, y, z = np.ogrid[:shape[0], :shape[1], :shape[2]]
    volume = np.zeros(shape, np.uint8)
    kidney = ((x - 256 * s[0]) / (150 * s[0])) ** 2 + ((y - 256 * s[1]) / (110 * s[1])) ** 2 + ((z - 128 * s[2]) / (70 * s[2])) ** 2 < 1
    volume[kidney] = 2
    volume[((x - 330 * s[0]) / (40 * s[0])) ** 2 + ((y - 300 * s[1]) / (40 * s[1])) ** 2 + ((z - 150 * s[2]) / (25 * s[2])) ** 2 < 1] = 3
    tree = np.zeros(shape, bool)
    grow(tree, np.array([120.0, 256.0, 128.0]) * s, np.array([1.0, 0.0, 0.0]), 100.0 * k, max(5.0 * k, 1.5), 3, np.random.RandomState(0))
    volume[tree & kidney] = 1
    return volume


def clock(fn):
    t0 = time.perf_counter(); out = fn()
    return out, 1e3 * (time.perf_counter() - t0)


SPACING = (0.75, 0.75, 1.5)
AFFINE = np.diag(SPACING + (1.0,))
volume, small = scene(SHAPE), scene(CHECK)
say("volume %s, spacing %s: %d kidney, %d artery, %d tumour voxels" % (SHAPE, SPACING, int((volume == 2).sum()),
                                                                          int((volume == 1).sum()), int((volume == 3).sum())))
host_small, ms_small_driver = clock(lambda: trainer.vessel_territories_case({'pred': small, 'affine': AFFINE}, 1, 2, other=3,
                                                                             return_labels=True))
small_skel = transform._skeleton_numpy(small == 1)[0]
(small_index, small_sq), ms_small_nearest = clock(lambda: transform._nearest_site_numpy(small_skel, SPACING))
say("host route at %s (the numpy twins): nearest %.1f ms, the whole driver %.1f ms (%d branches, %d centreline voxels)"
    % (CHECK, ms_small_nearest, ms_small_driver, host_small['branches'], int(small_skel.sum())))
if args.host_only:
    sys.exit(0)

import distance, morphology, skeleton
dev = torch.device("cuda:0")


def timed(fn, load):
    """Median over REPS of fn, each pass straight after an untimed `load` that keeps the clocks up; pass 0 warms up."""
    out, ms = None, []
    for rep in range(REPS + 1):
        load(); torch.cuda.synchronize()
        t0 = time.perf_counter(); out = fn(); torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    return out, float(np.median(ms[1:])), ms[1:]


# the quarter-resolution scene: both routes, equal
d_small = torch.from_numpy(small).to(dev)
sites_small = morphology.pack(torch.from_numpy(small_skel).to(dev))
load_small = lambda: distance.edt_squared(sites_small, SPACING)
(di, ds), ms_dev_small_nearest, _ = timed(lambda: territory.nearest(sites_small, SPACING), load_small)
assert torch.equal(di.cpu(), torch.from_numpy(small_index)) and torch.equal(ds.cpu(), torch.from_numpy(small_sq))
dev_small, ms_dev_small_driver, _ = timed(lambda: trainer.vessel_territories_case({'pred': d_small, 'affine': AFFINE}, 1, 2, other=3,
                                                                                  return_labels=True), load_small)
assert torch.equal(dev_small.pop('labels').cpu(), torch.from_numpy(host_small.pop('labels')))
assert json.dumps(dev_small, sort_keys=True) == json.dumps(host_small, sort_keys=True)
say("device route at %s, equal to the host route: nearest %.3f ms, the whole driver %.3f ms"
    % (CHECK, ms_dev_small_nearest, ms_dev_small_driver))

# the full size
d_volume = torch.from_numpy(volume).to(dev)
vessel = morphology.pack(d_volume, 'eq', 1)
skel = skeleton.thin(vessel)
g = skeleton.graph(skel, vessel, SPACING)
region = trainer._packed_union(d_volume, (2, 3))
tumour = morphology.unpack(morphology.pack(d_volume, 'eq', 3))
site_ids, K = territory.branch_sites(g)
load = lambda: distance.edt_squared(skel, SPACING)
sq_edt, ms_edt, all_edt = timed(lambda: distance.edt_squared(skel, SPACING), load)
(index, sq), ms_nearest, all_nearest = timed(lambda: territory.nearest(skel, SPACING), load)
_, ms_nearest_index, _ = timed(lambda: territory.nearest(skel, SPACING, return_sq=False), load)
assert torch.equal(sq, sq_edt)


def assign_tally():
    labels = territory.assign(skel, site_ids, index, region)
    return labels, territory.tally(labels, K, tumour, 1, region)


(labels, table), ms_assign_tally, _ = timed(assign_tally, load)
_, ms_driver, _ = timed(lambda: trainer.vessel_territories_case({'pred': d_volume, 'affine': AFFINE}, 1, 2, other=3), load)
_, ms_thin, _ = timed(lambda: skeleton.thin(vessel), load)

skel_np = morphology.unpack(skel).cpu().numpy().astype(bool)
(_, h_feature), ms_scipy = clock(lambda: ndi.distance_transform_edt(~skel_np, sampling=SPACING, return_indices=True))
h_index = index.cpu().numpy()
region_np = np.isin(volume, (2, 3))
h_labels, ms_h_assign = clock(lambda: transform._site_assign_numpy(skel_np, site_ids.cpu().numpy(), h_index, region_np))
h_table, ms_h_tally = clock(lambda: transform._territory_tally_numpy(h_labels, K, (volume == 3).astype(np.uint8), 1, region_np))
assert torch.equal(labels.cpu(), torch.from_numpy(h_labels)) and torch.equal(table.cpu(), torch.from_numpy(h_table))
every4 = np.zeros(SHAPE, bool)
every4[::4, ::4, ::4] = True                                                # scipy's site is as near as ours, whichever it takes
assert (trainer._contract_sq_numpy(every4, h_feature, SPACING) == sq.cpu().numpy()[every4]).all()
voxels = float(np.prod(SHAPE))
say("%d centreline voxels, %d branches, %d nodes; %d of %d region voxels in territories" % (
    g['n'], g['branches'], g['nodes'], int(h_table[1:].sum()), int(h_table.sum())))
say("device route at %s (median of %d passes after a warm-up pass, each after an untimed edt_squared)" % (SHAPE, REPS))
say("  %-34s %10.3f ms   (min %.3f, max %.3f)" % ("distance.edt_squared", ms_edt, min(all_edt), max(all_edt)))
say("  %-34s %10.3f ms   (min %.3f, max %.3f)" % ("territory.nearest (index and sq)", ms_nearest, min(all_nearest), max(all_nearest)))
say("  %-34s %10.3f ms" % ("territory.nearest (index only)", ms_nearest_index))
say("  %-34s %10.3f ms" % ("territory.assign + tally", ms_assign_tally))
say("  %-34s %10.3f ms" % ("skeleton.thin (inside the driver)", ms_thin))
say("  %-34s %10.3f ms" % ("trainer.vessel_territories_case", ms_driver))
say("nearest / edt_squared = %.2f (12 / 8 bytes per voxel and pass = 1.50); nearest writes, reads and writes 12 bytes a "
    "voxel, %.2f GB: %.0f GB/s" % (ms_nearest / ms_edt, 36 * voxels / 1e9, 36 * voxels / 1e6 / ms_nearest))
say("host route at %s (once)" % (SHAPE,))
say("  %-34s %10.1f ms   (scipy.ndimage.distance_transform_edt, return_indices)" % ("feature transform", ms_scipy))
say("  %-34s %10.1f ms   (the twins, equal to the device)" % ("assign + tally", ms_h_assign + ms_h_tally))
say(json.dumps({"shape": SHAPE, "check_shape": CHECK, "spacing": SPACING, "reps": REPS,
                "device_ms": {"edt_squared": round(ms_edt, 3), "nearest": round(ms_nearest, 3),
                              "nearest_index_only": round(ms_nearest_index, 3), "assign_tally": round(ms_assign_tally, 3),
                              "thin": round(ms_thin, 3), "driver": round(ms_driver, 3)},
                "nearest_over_edt": round(ms_nearest / ms_edt, 3),
                "host_ms": {"scipy_feature_transform": round(ms_scipy, 1), "assign_tally": round(ms_h_assign + ms_h_tally, 1)},
                "check_ms": {"host_nearest": round(ms_small_nearest, 1), "host_driver": round(ms_small_driver, 1),
                             "device_nearest": round(ms_dev_small_nearest, 3), "device_driver": round(ms_dev_small_driver, 3)},
                "identical_outputs": True}))
out = os.environ.get("RU3D_OUT")
path = os.path.join(out, os.path.basename(OUT)) if out else OUT
with open(path, "w") as f:
    f.write("\n".join(lines) + "\n")
