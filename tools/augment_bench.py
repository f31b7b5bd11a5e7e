"""Throughput of the on-device patch sampling / augmentation (GPU box): python tools/augment_bench.py [--spatial] [--degrade]
(--spatial adds a row for the same batch with rotation and elastic deformation switched on, --degrade one with Gaussian
noise, Gaussian blur and simulated low resolution forced on for every patch)."""
import os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "3d-unet-renal-anatomy-extraction_amd"))
import augment
dev = torch.device("cuda:0")
rng = np.random.RandomState(0)
cases = [augment.DeviceCase(rng.randn(256, 256, 160, 1).astype(np.float32), (rng.rand(256, 256, 160) * 4).astype(np.uint8), dev)
         for _ in range(2)]


def measure(aug, what, n=50, repeats=5):
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
