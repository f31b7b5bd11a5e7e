"""Local thickness at the size of a kidney CT: the synthetic 512x512x256 label volume of tools/territory_bench.py (a
kidney-sized ellipsoid, label 2; a branching arterial tree of three generations inside it, label 1; a spherical tumour,
label 3) on thickness.local_squared, stage by stage,
  lumen        the vessel mask (label 1): a thin, sparse mask of small balls - the calibre volume,
  parenchyma   the kidney without the lumen and the tumour (label 2): few millions of candidates, large balls,
each reporting thickness.inscribed_squared, the candidate list and its sort, the paint with presort on and off (the same
bytes, asserted), the two work counters of each order, the paint's tests per second and atomic bytes per second (8 bytes
an atomic), the cost model `sum over p of the voxels of ball(p)` evaluated from R2 on the device, and
distance.edt_squared on the same mask in the same run as the yardstick: the transform the feature necessarily contains,
so the ratio says what the paint adds.  Device times are medians of REPS passes after a warm-up pass, each pass between
synchronises straight after an untimed edt_squared that keeps the clocks up; the two painting orders alternate inside a
pass.  Every stage is a child process of its own under its own time limit (--limit seconds); a stage that runs into it
is reported as such and no later stage is started.  At --check-shape (a quarter of the resolution) the lumen is asserted
equal to the numpy twin first.  Prints one line per figure and a JSON summary line per stage, and writes the same text to
profiles/thickness_512x512x256.txt.  `--host-only` builds the scenes and runs the host parts."""
import argparse, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "3d-unet-renal-anatomy-extraction_amd"))
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--shape", type=int, nargs=3, default=(512, 512, 256))
ap.add_argument("--check-shape", type=int, nargs=3, default=(128, 128, 64))
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--limit", type=int, default=240, help="seconds a stage may take")
ap.add_argument("--stage", choices=("check", "lumen", "parenchyma"), help="run this stage in this process (the parent's children)")
ap.add_argument("--host-only", action="store_true")
args = ap.parse_args()
SHAPE, CHECK, REPS = tuple(args.shape), tuple(args.check_shape), args.reps
OUT = os.path.join(ROOT, "profiles", "thickness_%dx%dx%d.txt" % SHAPE)
SPACING = (0.75, 0.75, 1.5)
LABEL = {"lumen": 1, "parenchyma": 2}


def say(text):
    print(text, flush=True)


def tube(volume, a, b, radius):
    """Set the voxels within `radius` of the segment a - b."""
    lo = np.maximum(np.floor(np.minimum(a, b) - radius).astype(int), 0)
    hi = np.minimum(np.ceil(np.maximum(a, b) + radius).astype(int) + 1, volume.shape)
    p = np.stack(np.meshgrid(*[np.arange(l, h) for l, h in zip(lo, hi)], indexing="ij"), axis=-1).astype(float)
    t = np.clip(((p - a) * (b - a)).sum(-1) / ((b - a) ** 2).sum(), 0, 1)
    volume[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] |= ((p - (a + t[..., None] * (b - a))) ** 2).sum(-1) <= radius * radius


def branch(volume, start, direction, length, radius, depth, rng):
    end = start + direction * length
    tube(volume, start, end, radius)
    if depth:
        for sign in (-1, 1):
            turn = np.cross(direction, rng.randn(3))
            d = direction + 0.9 * sign * turn / np.linalg.norm(turn)
            branch(volume, end, d / np.linalg.norm(d), length * 0.7, max(radius * 0.7, 1.5), depth - 1, rng)


def scene(shape):
    """uint8 label volume of `shape`, the scene of tools/territory_bench.py: kidney 2, arterial tree 1, tumour 3."""
    s = np.array(shape, float) / (512.0, 512.0, 256.0)
    k = float(s.min())
    x, y, z = np.ogrid[:shape[0], :shape[1], :shape[2]]
    volume = np.zeros(shape, np.uint8)
    kidney = ((x - 256 * s[0]) / (150 * s[0])) ** 2 + ((y - 256 * s[1]) / (110 * s[1])) ** 2 + ((z - 128 * s[2]) / (70 * s[2])) ** 2 < 1
    volume[kidney] = 2
    volume[((x - 330 * s[0]) / (40 * s[0])) ** 2 + ((y - 300 * s[1]) / (40 * s[1])) ** 2 + ((z - 150 * s[2]) / (25 * s[2])) ** 2 < 1] = 3
    tree = np.zeros(shape, bool)
    branch(tree, np.array([120.0, 256.0, 128.0]) * s, np.array([1.0, 0.0, 0.0]), 100.0 * k, max(5.0 * k, 1.5), 3, np.random.RandomState(0))
    volume[tree & kidney] = 1
    return volume


def median(ms):
    return float(np.median(ms))


def stage_check():
    """the quarter-resolution lumen: the device equal to the numpy twin, both painting orders"""
    import torch, morphology, thickness, transform
    dev = torch.device("cuda:0")
    small = scene(CHECK) == 1
    t0 = time.perf_counter(); want = transform._local_thickness_numpy(small, SPACING); host_ms = 1e3 * (time.perf_counter() - t0)
    p = morphology.pack(torch.from_numpy(small.astype(np.uint8)).to(dev))
    for presort in (True, False):
        assert np.array_equal(thickness.local_squared(p, SPACING, presort=presort).cpu().numpy(), want)
    say("lumen at %s (%d voxels): device equal to the numpy twin in both painting orders; the twin took %.0f ms on the host"
        % (CHECK, int(small.sum()), host_ms))


def stage_mask(name):
    import torch, distance, morphology, thickness
    dev = torch.device("cuda:0")
    volume = scene(SHAPE)
    mask = morphology.pack(torch.from_numpy(volume).to(dev), 'eq', LABEL[name])
    X, Y, Z = SHAPE
    load = lambda: distance.edt_squared(mask, SPACING)

    def timed(fns, reps):
        """medians over `reps` passes of every fn of `fns`, alternating inside a pass, each straight after an untimed load"""
        ms, out = [[] for _ in fns], [None] * len(fns)
        for rep in range(reps + 1):
            for k, fn in enumerate(fns):
                load(); torch.cuda.synchronize()
                t0 = time.perf_counter(); out[k] = fn(); torch.cuda.synchronize()
                ms[k].append(1e3 * (time.perf_counter() - t0))
        return out, [m[1:] for m in ms]

    (sq_edt, r2), (ms_edt, ms_r2) = timed([lambda: distance.edt_squared(mask, SPACING),
                                           lambda: thickness.inscribed_squared(mask, SPACING)], REPS)
    (index,), (ms_list,) = timed([lambda: thickness.candidates(mask)], REPS)
    (ordered,), (ms_sort,) = timed([lambda: thickness.sort_candidates(r2, index)], REPS)
    n = int(index.numel())
    radius = torch.sqrt(r2.reshape(-1)[index.to(torch.int64)])
    voxel = SPACING[0] * SPACING[1] * SPACING[2]
    model = float((4.0 / 3.0 * np.pi * radius ** 3 / voxel).sum().item())
    boxes = float(((2 * torch.floor(radius / SPACING[0]) + 3) * (2 * torch.floor(radius / SPACING[1]) + 3)
                   * (2 * torch.floor(radius / SPACING[2]) + 3)).sum().item())
    top = torch.sort(radius, descending=True).values
    share = float((top[:max(n // 100, 1)] ** 3).sum().item() / max(float((top ** 3).sum().item()), 1e-300))
    say("%s: %d candidates, radius %.2f mm mean, %.2f mm max; cost model sum of ball volumes %.4g voxels (unclipped boxes "
        "%.4g); the largest 1 %% of the balls hold %.1f %% of it" % (name, n, float(radius.mean().item()), float(top[0].item()),
                                                                     model, boxes, 100 * share))
    say("  %-38s %10.3f ms   (min %.3f, max %.3f)" % ("distance.edt_squared (yardstick)", median(ms_edt), min(ms_edt), max(ms_edt)))
    say("  %-38s %10.3f ms" % ("thickness.inscribed_squared", median(ms_r2)))
    say("  %-38s %10.3f ms   (one host read of the count)" % ("thickness.candidates", median(ms_list)))
    say("  %-38s %10.3f ms" % ("thickness.sort_candidates", median(ms_sort)))
    # one pass of each order first, on its own and announced, so that a time limit tells which order ran into it
    work, first = {}, {}
    for presort, lst in ((True, ordered), (False, index)):
        load(); torch.cuda.synchronize()
        t0 = time.perf_counter(); out, w = thickness.paint(r2, lst, SHAPE, SPACING, count_work=True); torch.cuda.synchronize()
        first[presort] = 1e3 * (time.perf_counter() - t0)
        work[presort] = [int(v) for v in w.tolist()]
        say("  paint presort=%-5s first pass %10.3f ms: %d voxels tested, %d atomics issued" % (presort, first[presort], *work[presort]))
        if presort:
            want = out
        else:
            assert torch.equal(out.view(torch.int64), want.view(torch.int64)), "the two painting orders differ"
    reps = REPS if max(first.values()) < 2000 else 2
    (_, _), (ms_on, ms_off) = timed([lambda: thickness.paint(r2, ordered, SHAPE, SPACING)[0],
                                     lambda: thickness.paint(r2, index, SHAPE, SPACING)[0]], reps)
    (_,), (ms_whole,) = timed([lambda: thickness.local_squared(mask, SPACING)], reps)
    summary = {"stage": name, "shape": SHAPE, "spacing": SPACING, "reps": reps, "candidates": n, "cost_model_voxels": model,
               "identical_orders": True,
               "device_ms": {"edt_squared": round(median(ms_edt), 3), "inscribed_squared": round(median(ms_r2), 3),
                             "candidates": round(median(ms_list), 3), "sort": round(median(ms_sort), 3),
                             "paint_presort": round(median(ms_on), 3), "paint_element_order": round(median(ms_off), 3),
                             "local_squared": round(median(ms_whole), 3)}}
    for presort, ms in ((True, ms_on), (False, ms_off)):
        tested, issued = work[presort]
        t = median(ms)
        say("  %-38s %10.3f ms   (min %.3f, max %.3f; %d passes): %.3g tests/s, %.3g atomic bytes/s"
            % ("paint, presort=%s" % presort, t, min(ms), max(ms), len(ms), tested / t * 1e3, 8.0 * issued / t * 1e3))
        summary["presort" if presort else "element_order"] = {"tested": tested, "atomics": issued,
                                                              "tests_per_s": tested / t * 1e3,
                                                              "atomic_bytes_per_s": 8.0 * issued / t * 1e3}
    say("  %-38s %10.3f ms   = %.1f x edt_squared" % ("thickness.local_squared (whole)", median(ms_whole),
                                                      median(ms_whole) / median(ms_edt)))
    say("  tested / cost model = %.2f; atomics sorted / element order = %.3f" % (work[True][0] / max(model, 1.0),
                                                                                 work[True][1] / max(work[False][1], 1)))
    say(json.dumps(summary))


if args.stage:
    stage_check() if args.stage == "check" else stage_mask(args.stage)
    sys.exit(0)

lines = []
volume = scene(SHAPE)
lines.append("volume %s, spacing %s: %d kidney, %d artery, %d tumour voxels" % (SHAPE, SPACING, int((volume == 2).sum()),
                                                                               int((volume == 1).sum()), int((volume == 3).sum())))
print(lines[-1], flush=True)
if args.host_only:
    sys.exit(0)
lines.append("device route (medians of %d passes after a warm-up pass, each after an untimed edt_squared; every stage a process "
             "of its own under a limit of %d s)" % (REPS, args.limit))
for stage in ("check", "lumen", "parenchyma"):
    cmd = [sys.executable, os.path.abspath(__file__), "--stage", stage, "--reps", str(REPS), "--shape", *map(str, SHAPE),
           "--check-shape", *map(str, CHECK)]
    try:
        done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=args.limit)
        text, rc = done.stdout, done.returncode
    except subprocess.TimeoutExpired as e:
        text, rc = (e.stdout.decode() if isinstance(e.stdout, bytes) else (e.stdout or "")), None
    kept = [l for l in text.splitlines() if not l.startswith("/opt/amdgpu")]
    print("\n".join(kept), flush=True)
    lines += kept
    if rc != 0:
        lines.append("stage %s %s: no later stage was started" % (stage, "ran into its limit of %d s" % args.limit if rc is None
                                                                  else "ended with status %d" % rc))
        print(lines[-1], flush=True)
        break
out = os.environ.get("RU3D_OUT")
path = os.path.join(out, os.path.basename(OUT)) if out else OUT
with open(path, "w") as f:
    f.write("\n".join(lines) + "\n")
sys.exit(0 if rc == 0 else 1)
