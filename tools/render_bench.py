#!/usr/bin/env python3
"""Rendering on a synthetic 512 x 512 x 256 case, device route against numpy route (run on the MI355X):

    python tools/render_bench.py [--repeats 7] [--host-size 96]

Times `visualize.case_sheet` (24 tiles, one ru3d_render_tiles launch, window given so that no percentile is taken) and
`visualize.render_case` (four 768^2 views, translucent kidney) end to end - launch, kernel, download, a host clock
around calls that end in a device-to-host copy - after a warm-up, and reports the median of `--repeats` runs each.  The
numpy route is the definition and is slow: it is timed once, for the sheet at full size and for ONE view at
`--host-size` pixels, and its figure is scaled by the pixel count for the comparison (said so in the output).
Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "3d-unet-renal-anatomy-extraction_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--host-size", type=int, default=96)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("render_bench: needs a HIP device (a CPU timing says nothing about the MI355X)")
    import visualize as V
    dev = torch.device("cuda:0")
    shape, spacing = (512, 512, 256), (0.78, 0.78, 1.5)
    g = [torch.arange(n, device=dev, dtype=torch.float32) for n in shape]
    volume = torch.zeros(shape, dtype=torch.uint8, device=dev)
    for label, (cx, cy, cz, r) in ((1, (256, 250, 128, 110)), (2, (280, 270, 140, 45)), (3, (220, 230, 110, 25))):
        d2 = ((g[0] - cx) * spacing[0])[:, None, None] ** 2 + ((g[1] - cy) * spacing[1])[None, :, None] ** 2 \
            + ((g[2] - cz) * spacing[2])[None, None, :] ** 2
        volume[d2 <= float(r * r) * spacing[0] ** 2] = label
    torch.manual_seed(0)
    image = torch.randn(shape + (1,), device=dev) * 40 + 100 * (volume[..., None] > 0)
    case = {"image": image, "label": volume, "pred": torch.roll(volume, (3, -2, 1), (0, 1, 2)),
            "affine": np.diag(list(spacing) + [1.0])}
    views = ((30, 20), (120, 20), (210, -20), (300, 60))

    def sheet():
        return V.case_sheet(case, num_slices=8, window=(-80.0, 220.0))

    def shots():
        return V.render_case(case, views=views, size=768, alpha={1: 0.35})

    props = torch.cuda.get_device_properties(0)
    out = {"device": torch.cuda.get_device_name(0), "arch": getattr(props, "gcnArchName", ""),
           "compute_units": props.multi_processor_count, "volume": list(shape), "repeats": args.repeats}
    for name, fn in (("sheet_24_tiles", sheet), ("views_4x768", shots)):
        fn()
        fn()
        times = []
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            result = fn()
            times.append((time.perf_counter() - t0) * 1e3)
        out[name + "_device_ms_median"] = round(statistics.median(times), 3)
        out[name + "_device_ms_min_max"] = [round(min(times), 3), round(max(times), 3)]
        out[name + "_shape"] = list(result.shape)
    host = {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in case.items()}
    t0 = time.perf_counter()
    host_sheet = V.case_sheet(host, num_slices=8, window=(-80.0, 220.0))
    out["sheet_24_tiles_numpy_ms_once"] = round((time.perf_counter() - t0) * 1e3, 1)
    out["sheet_equal"] = bool(np.array_equal(host_sheet, sheet()))
    t0 = time.perf_counter()
    small = V.render_case(host, views=views[:1], size=args.host_size, alpha={1: 0.35})
    once = (time.perf_counter() - t0) * 1e3
    out["view_numpy_ms_once_at_%d" % args.host_size] = round(once, 1)
    out["views_4x768_numpy_ms_scaled_by_pixels"] = round(once * 4 * (768 / args.host_size) ** 2, 1)
    out["view_equal_at_%d" % args.host_size] = bool(np.array_equal(
        small, V.render_case(case, views=views[:1], size=args.host_size, alpha={1: 0.35})))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
