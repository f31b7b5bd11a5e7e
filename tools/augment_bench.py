"""Throughput of the on-device patch sampling / augmentation (GPU box): python tools/augment_bench.py [--spatial] [--degrade]
[--oversample] (--spatial adds a row for the same batch with rotation and elastic deformation switched on, --degrade one
with Gaussian noise, Gaussian blur and simulated low resolution forced on for every patch, --oversample the build time of
the class-location index next to its numpy twin and, on a case whose class 3 is one ball of radius 6, the batch with
enforce_label_indices=[3] next to the batch with oversample_foreground=1.0, foreground_classes=[3])."""
import os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "3d-unet-renal-anatomy-extraction_amd"))
import augment
dev = torch.device("cuda:0")
rng = np.random.RandomState(0)
cases = [augment.DeviceCase(rng.randn(256, 256, 160, 1).astype(np.float32), (rng.rand(256, 256, 160) * 4).astype(np.uint8), dev)
         for _ in range(2)]


def measure(aug, what, n=50, repeats=5, cases=cases):
    """Warm-up, then the median over `repeats` timed windows of `n` batches, each window closed by a device synchronise."""
    for _ in range(3):
        aug.batch(cases, 2)
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(n):
            aug.batch(cases, 2)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) / n)
    dt = float(np.median(times))
    print("batch of 2 x 128^3 patches (%s): %.3f ms = %.0f M voxels/s  [min %.3f, max %.3f ms over %d windows of %d]"
          % (what, 1e3 * dt, 2 * 128 ** 3 / dt / 1e6, 1e3 * min(times), 1e3 * max(times), repeats, n))


np.random.seed(0)
measure(augment.DeviceAugment(scale=0.1, crop_size=128, crop_mode="random"),
        "rescale-crop + mirror + contrast + brightness + gamma")
if "--spatial" in sys.argv[1:]:
    # the same batch through the free-form transform: the training script's rotation about x, elastic deformation on
    measure(augment.DeviceAugment(scale=0.1, crop_size=128, crop_mode="random",
                                  rotation=((-0.1 * np.pi, 0.1 * np.pi), (0, 0), (0, 0)), elastic_spacing=16,
                                  elastic_magnitude=(0, 8)),
            "rotation + rescale + elastic g=16 + mirror + contrast + brightness + gamma")
if "--degrade" in sys.argv[1:]:
    # the same batch with the three image-quality ops on every patch (p = 1), at the usual recipe's parameter ranges
    measure(augment.DeviceAugment(scale=0.1, crop_size=128, crop_mode="random", noise=(1.0, (0, 0.1)),
                                  blur=(1.0, (0.5, 1.0)), low_res=(1.0, (0.5, 1.0))),
            "rescale-crop + mirror + noise + blur + low-res + contrast + brightness + gamma")
if "--oversample" in sys.argv[1:]:
    import transform
    g = np.meshgrid(np.arange(256), np.arange(256), np.arange(160), indexing="ij")
    label = (rng.rand(256, 256, 160) * 3).astype(np.uint8)                      # 0 .. 2 everywhere
    label[(g[0] - 70) ** 2 + (g[1] - 180) ** 2 + (g[2] - 40) ** 2 <= 36] = 3      # one ball of radius 6
    ball = [augment.DeviceCase(rng.randn(256, 256, 160, 1).astype(np.float32), label, dev)]
    print("class 3: %d of %d voxels" % (int((label == 3).sum()), label.size))
    times = []
    for _ in range(7):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        index = augment.ClassIndex(ball[0].label, 10000)                         # the call and its two downloads
        times.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    counts = transform.class_locations(label, 10000)[0]
    host = time.perf_counter() - t0
    assert np.array_equal(counts, index.counts)
    print("class-location index of 256 x 256 x 160 uint8, 10000 per class: device %.3f ms (median of 7, min %.3f), "
          "transform.class_locations on the host %.0f ms" % (1e3 * float(np.median(times)), 1e3 * min(times), 1e3 * host))
    # the plain and the enforce rows run code the index does not touch: the parent commit's numbers, taken in this run
    np.random.seed(0)
    measure(augment.DeviceAugment(scale=0.1, crop_size=128, crop_mode="random"), "one-ball case, plain", cases=ball)
    np.random.seed(0)
    measure(augment.DeviceAugment(scale=0.1, crop_size=128, crop_mode="random", enforce_label_indices=[3]),
            "one-ball case, enforce_label_indices=[3]", n=20, cases=ball)
    np.random.seed(0)
    measure(augment.DeviceAugment(scale=0.1, crop_size=128, crop_mode="random", oversample_foreground=1.0,
                                  foreground_classes=[3]),
            "one-ball case, oversample_foreground=1.0, foreground_classes=[3]", cases=ball)
    print("the enforce row depends on the structure's size (the smaller, the more tries); the oversampled row does not")
