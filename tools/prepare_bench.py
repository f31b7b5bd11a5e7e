"""Per-stage times of the preparation of one case on both routes: a synthetic 512x512x256 CT-like case (a body-shaped
blob in air, a three-class label) through the stages of data.orient_crop_case, data.analyze_cases and
data.resample_normalize_case, once with numpy / scipy on the host and once with csrc/prepare.hip + csrc/augment.hip on
the device.  Stages: the non-air box, the masked sample of the case (`[::10]` and every voxel), the seven statistics
over a pooled sample of ~10^7 values, the image zoom and the label zoom; upload and download of the case are stated
separately - and so is writing and reading the case as .nii.gz, which stays on the host on either route and is what a
real run waits for.  Device stages are timed between synchronises after a warm-up pass, median of REPS passes; the host
route runs once (it takes seconds).  The routes' outputs are compared by the contracts of tests/test_gpu_prepare.py
before anything is printed.  Prints one line per stage and a JSON summary line.  `--device-only` skips the files, the host
route and the comparison: the run to put under `rocprofv3 --kernel-trace --stats` (tools/kstats.py summarises it)."""
import json, os, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "3d-unet-renal-anatomy-extraction_amd"))
import numpy as np, torch, augment, data, prepare, transform
dev = torch.device("cuda:0")
SHAPE, AIR, POOL, REPS = (512, 512, 256), -200, 10_000_000, 7
TARGET_SCALE = (0.5, 0.5, 0.8)                       # 0.78 x 0.78 x 2.4 mm -> 1.56 x 1.56 x 3 mm
DEVICE_ONLY = "--device-only" in sys.argv
rng = np.random.RandomState(0)
x, y, z = np.ogrid[:SHAPE[0], :SHAPE[1], :SHAPE[2]]


def blob(c, r):
    return ((x - c[0]) / float(r[0])) ** 2 + ((y - c[1]) / float(r[1])) ** 2 + ((z - c[2]) / float(r[2])) ** 2 < 1


image = np.full(SHAPE, -1000.0, np.float32)
body = blob((256, 250, 128), (200, 150, 140))
image[body] = np.round(rng.randn(int(body.sum())) * 60 + 40).astype(np.float32)
label = np.zeros(SHAPE, np.uint8)
for c in ((170, 260, 120), (340, 250, 130)):
    label[blob(c, (50, 60, 45))] = 1
    label[blob((c[0] + 10, c[1], c[2]), (20, 25, 15))] = 2
image = image[..., None]
out_shape = tuple(int(round(s * f)) for s, f in zip(SHAPE, TARGET_SCALE))
pooled = np.round(rng.randn(POOL) * 80 + 100).astype(np.float32)
times = {"host": {}, "device": {}}


def host(stage, fn):
    t0 = time.perf_counter(); out = fn()
    times["host"][stage] = 1e3 * (time.perf_counter() - t0)
    return out


def device(stage, fn):
    torch.cuda.synchronize(); t0 = time.perf_counter(); out = fn(); torch.cuda.synchronize()
    times["device"].setdefault(stage, []).append(1e3 * (time.perf_counter() - t0))
    return out


def host_box():
    pos = np.array(np.where(image[..., 0] > AIR))
    return np.array([pos.min(axis=1), pos.max(axis=1)]).T


# ---- files: the same on either route
with tempfile.TemporaryDirectory() as tmp:
    case = {"case_id": "bench", "affine": np.diag([0.78, 0.78, 2.4, 1.0]), "image": image, "label": label}
    DEVICE_ONLY or host("files: save_case (.nii.gz)", lambda: data.save_case(case, tmp))
    DEVICE_ONLY or host("files: load_case (.nii.gz)", lambda: data.load_case(os.path.join(tmp, "bench.image.nii.gz"),
                                                                             os.path.join(tmp, "bench.label.nii.gz")))

# ---- host route
if not DEVICE_ONLY:
    h_box = host("non-air box", host_box)
    h_s10 = host("masked sample [::10]", lambda: image[..., 0][label > 0][::10])
    h_s1 = host("masked sample [::1]", lambda: image[..., 0][label > 0])
    h_stats = host("statistics of 1e7 pooled values", lambda: data._intensity_statistics(pooled))
    h_img = host("image zoom", lambda: transform.rescale(image, TARGET_SCALE, multi_class=True))
    h_lab = host("label zoom (3 classes)", lambda: transform.rescale(label.astype(np.int64), TARGET_SCALE, is_label=True))

# ---- device route
d_image = device("upload (image fp32 + label uint8)", lambda: torch.from_numpy(image).to(dev))
d_label = torch.from_numpy(label).to(dev)
d_pooled = torch.from_numpy(pooled).to(dev)
for rep in range(REPS + 1):
    d_box = device("non-air box", lambda: prepare.threshold_bbox(d_image, AIR)[0])
    d_s10 = device("masked sample [::10]", lambda: prepare.masked_sample(d_image, d_label, 0, 10))
    d_s1 = device("masked sample [::1]", lambda: prepare.masked_sample(d_image, d_label, 0, 1))
    d_stats = device("statistics of 1e7 pooled values", lambda: prepare.intensity_statistics(d_pooled))
    d_img = device("image zoom", lambda: augment.resample_image(d_image, out_shape))
    d_lab = device("label zoom (3 classes)", lambda: augment.resample_label(d_label, out_shape))
    d_up = device("upload (image fp32 + label uint8)", lambda: (torch.from_numpy(image).to(dev), torch.from_numpy(label).to(dev)))
    d_down = device("download (zoomed image + label)", lambda: (d_img.cpu(), d_lab.to(torch.uint8).cpu()))
    if rep == 0:
        times["device"] = {}                         # warm-up pass: code objects, allocator

if not DEVICE_ONLY:
    assert np.array_equal(d_box, h_box)
    assert np.array_equal(d_s10.cpu().numpy(), h_s10) and np.array_equal(d_s1.cpu().numpy(), h_s1)
    for k in ("median", "min", "max", "pct_00_5", "pct_99_5"):
        assert d_stats[k] == h_stats[k], (k, d_stats[k], h_stats[k])
    for k in ("mean", "std"):
        assert abs(d_stats[k] - h_stats[k]) <= 1e-5 * abs(h_stats[k]), (k, d_stats[k], h_stats[k])
    assert np.abs(d_img.cpu().numpy() - h_img).max() <= 2e-3      # test_gpu_augment.py's 2e-6 on unit-range data, times the range of 1000
    assert (d_lab.cpu().numpy() != h_lab).mean() <= 2e-3

summary = {"shape": list(SHAPE), "zoomed_shape": list(out_shape), "pooled_values": POOL,
           "foreground_voxels": int((label > 0).sum()), "reps": REPS, "ms": {}}
for stage in list(times["host"]) + [s for s in times["device"] if s not in times["host"]]:
    h = times["host"].get(stage)
    d = float(np.median(times["device"][stage])) if stage in times["device"] else None
    summary["ms"][stage] = {"host": None if h is None else round(h, 3), "device": None if d is None else round(d, 3)}
    print("%-36s host %10s ms   device %10s ms" % (stage, "-" if h is None else "%.2f" % h, "-" if d is None else "%.3f" % d))
print(json.dumps(summary))
