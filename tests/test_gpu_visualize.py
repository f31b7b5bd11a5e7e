"""The render kernels (csrc/render.hip) and the device route of visualize against the numpy route, which restates the
contract of include/ru3d.h: panels, ranges, sheets, pictures and depth images equal with ==, no tolerances.
`-m gpu` only."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no HIP device", allow_module_level=True)

import _native as N  # noqa: E402
import network  # noqa: E402
import trainer as T  # noqa: E402
import visualize as V  # noqa: E402

DEV = torch.device("cuda:0")


def _ball(shape, spacing, centre, radius):
    grid = np.indices(shape).astype(np.float64)
    return sum(((grid[c] + 0.5) * spacing[c] - centre[c] * shape[c] * spacing[c]) ** 2 for c in range(3)) <= radius * radius


def synthetic_case(shape, spacing, seed):
    """An image, and a label / prediction of three nested structures (kidney 1, tumour 2 and a duct 3 inside it)."""
    rng = np.random.default_rng(seed)
    reach = min(shape[c] * spacing[c] for c in range(3))
    label = np.zeros(shape, dtype=np.uint8)
    label[_ball(shape, spacing, (0.5, 0.45, 0.5), 0.4 * reach)] = 1
    label[_ball(shape, spacing, (0.55, 0.5, 0.45), 0.18 * reach)] = 2
    label[_ball(shape, spacing, (0.4, 0.4, 0.6), 0.1 * reach)] = 3
    pred = np.roll(label, (2, -1, 1), axis=(0, 1, 2))
    pred[rng.random(shape) < 0.001] = 2
    image = (rng.normal(size=shape + (1,)) * 40 + 100 * (label[..., None] > 0)).astype(np.float32)
    affine = np.diag(list(spacing) + [1.0])
    return {"image": image, "label": label, "pred": pred, "affine": affine}


def on_device(case):
    return {k: (torch.from_numpy(v).to(DEV) if k in ("image", "label", "pred") else v) for k, v in case.items()}


def test_case_panels_with_hip_operands_equal_the_numpy_route():
    rng = np.random.default_rng(0)
    image = rng.normal(size=(20, 18, 14, 2)).astype(np.float32)
    image[rng.random(image.shape) < 0.3] = 0.0                                # ties
    image[rng.random(image.shape) < 0.1] = -0.0                               # both zeros
    image[..., 1] = np.round(image[..., 1] * 2) / 2
    label = rng.integers(0, 4, size=(20, 18, 14)).astype(np.uint8)
    pred = rng.integers(0, 3, size=(20, 18, 14)).astype(np.uint8)
    for case, args in (({"image": image, "label": label, "pred": pred}, (0.5, 0)),
                       ({"image": image, "pred": pred}, (0.3, 1)),
                       ({"image": image, "label": np.eye(4, dtype=np.float32)[label],
                         "pred": np.eye(4, dtype=np.float32)[pred]}, (0.7, 2, True, True))):
        host_panels, host_ranges = V.case_panels(case, *args)
        panels, ranges = V.case_panels(on_device(case), *args)
        assert len(panels) == len(host_panels)
        for a, b in zip(panels, host_panels):
            assert isinstance(a, np.ndarray) and a.dtype == b.dtype and np.array_equal(a, b)
        assert len(ranges) == len(host_ranges)
        for a, b in zip(ranges, host_ranges):
            assert a[0] == b[0] and a[1] == b[1] and type(a[0]) is type(b[0])
    # a mixed case: only the image lives in HBM
    panels, ranges = V.case_panels({"image": torch.from_numpy(image).to(DEV), "label": label}, 0.5, 0)
    assert np.array_equal(panels[2], label[10]) and ranges[0] == [np.percentile(image, 0.5), np.percentile(image, 99.5)]


def test_case_plt_runs_with_hip_operands_under_agg():
    import matplotlib
    matplotlib.use("Agg", force=True)
    import matplotlib.pyplot as plt
    case = on_device(synthetic_case((24, 20, 12), (1.0, 1.0, 2.0), 1))
    before = len(plt.get_fignums())
    V.case_plt(case, 0.5, 2)
    assert len(plt.get_fignums()) == before + 1
    plt.close("all")


@pytest.mark.parametrize("shape,spacing", [((192, 160, 96), (0.78, 0.78, 3.0)), ((61, 45, 70), (1.2, 0.9, 1.7)),
                                           ((33, 31, 129), (1.0, 1.0, 0.5))])
def test_case_sheet_and_render_case_equal_the_numpy_route(shape, spacing):
    case = synthetic_case(shape, spacing, 2)
    dev = on_device(case)
    assert np.array_equal(V.case_sheet(dev, num_slices=4), V.case_sheet(case, num_slices=4))
    assert np.array_equal(V.case_sheet(dev, axes=(2, 0), num_slices=3, window=(-50.0, 150.0), pixel_mm=1.3),
                          V.case_sheet(case, axes=(2, 0), num_slices=3, window=(-50.0, 150.0), pixel_mm=1.3))
    only = {"pred": dev["pred"], "label": dev["label"], "affine": case["affine"]}
    assert np.array_equal(V.case_sheet(only, num_slices=3),
                          V.case_sheet({"pred": case["pred"], "label": case["label"], "affine": case["affine"]}, num_slices=3))
    views = ((0, 0), (33, 21), (200, -47), (90, 90))
    size = 96 if shape[0] > 100 else 64
    for kwargs in ({}, {"alpha": {1: 0.35}}, {"alpha": 0.5, "labels": (1, 3)}, {"labels": (2,), "colours": {2: (10, 250, 40)}}):
        got, got_depth = V.render_case(dev, views=views, size=size, return_depth=True, **kwargs)
        want, want_depth = V.render_case(case, views=views, size=size, return_depth=True, **kwargs)
        assert got_depth.dtype == np.int32 and np.array_equal(got_depth, want_depth)
        assert got.dtype == np.uint8 and np.array_equal(got, want)
        assert (want_depth >= 0).any()


def test_sheet_and_views_with_a_capped_grid():
    """ru3d_render_tiles launches 8 blocks a CU of the budget and deals 256-pixel chunks of the tiles over them;
    ru3d_render_surface_prepare caps its word loop at the same figure.  (96, 96, 96): 96 * 96 * 2 = 18432 words = 72 blocks
    uncapped, and the tiles of the 772 x 1030 sheet are some 3000 chunks - under a budget of 8 CUs there are 64 blocks for
    either (2048 with the whole chip), so the word loop makes a second trip and a block paints some 47 chunks.  The same
    bits as the numpy route, as in test_case_sheet_and_render_case_equal_the_numpy_route."""
    case = synthetic_case((96, 96, 96), (1.0, 1.0, 1.0), 4)
    dev = on_device(case)
    want_sheet = V.case_sheet(case, num_slices=4)
    assert want_sheet.shape[0] * want_sheet.shape[1] > 64 * 256
    views = ((33, 21), (200, -47))
    want, want_depth = V.render_case(case, views=views, size=64, return_depth=True)
    try:
        assert N.lib.ru3d_set_cu_budget(8) == 0
        sheet = V.case_sheet(dev, num_slices=4)
        got, got_depth = V.render_case(dev, views=views, size=64, return_depth=True)
    finally:
        N.lib.ru3d_set_cu_budget(0)
    assert N.lib.ru3d_get_cu_budget() == torch.cuda.get_device_properties(DEV).multi_processor_count
    assert np.array_equal(sheet, want_sheet)
    assert got_depth.dtype == np.int32 and np.array_equal(got_depth, want_depth) and np.array_equal(got, want)
    assert (want_depth >= 0).any()


@pytest.mark.parametrize("size", [15, 33, 65])
def test_axis_views_of_a_brick_aligned_box_with_plates_behind_brick_faces_equal_the_numpy_route(size):
    # cos(270 deg) and sin(180 deg) are not zero but far below an ulp of a coordinate, and with an odd size the middle
    # column starts one ulp from a brick face: the contract's rounded positions drift across the face and meet a plate
    # that a jump sized in real arithmetic would pass
    volume = np.zeros((32, 32, 96), dtype=np.uint8)
    volume[16, 13:15, 40:48] = 1
    volume[16, 17:19, 40:48] = 2
    volume[10:13, 16, 50:56] = 3
    volume[19:22, 15, 50:56] = 1
    volume[10:12, 20:22, 64] = 2
    volume[20:22, 10:12, 63] = 3
    volume[8, 8, 32] = 1
    volume[23, 23, 71] = 1
    views = ((270, 0), (90, 0), (180, 0), (0, 0), (0, 90), (0, -90), (270, 90), (180, -90))
    for spacing in ((1.0, 1.0, 1.0), (0.75, 0.75, 3.0)):
        case = {"pred": volume, "affine": np.diag(list(spacing) + [1.0])}
        dev = {"pred": torch.from_numpy(volume).to(DEV), "affine": case["affine"]}
        for alpha in (None, {1: 0.5}):
            got, got_depth = V.render_case(dev, views=views, size=size, alpha=alpha, return_depth=True)
            want, want_depth = V.render_case(case, views=views, size=size, alpha=alpha, return_depth=True)
            assert np.array_equal(got_depth, want_depth) and np.array_equal(got, want)
            assert (want_depth >= 0).any(axis=(1, 2)).all()
    # the hand-built ray: x one ulp below the face x = 16 and carried across it by rounding at n = 10
    table = V.colour_table()
    prepared = V._Prepared(torch.from_numpy(volume).to(DEV), table)
    view = V.fit_view(([8, 8, 32], [24, 24, 72]), (1.0, 1.0, 1.0), 270, 0, 1)
    for o0, d0 in ((np.nextafter(16.0, 0.0), 9e-17), (np.nextafter(16.0, 0.0), 3e-16), (16.0, -9e-17), (np.nextafter(16.0, 32.0), -4e-16)):
        hand = dict(view, o=np.array([o0, 8.25, 44.5]), dw=np.array([d0, 0.5, 0.0]), num_steps=60)
        got, got_depth = V.cast_device(prepared, hand, 1, 1)
        want, want_depth = V.cast_numpy(volume, table, hand, 1, 1)
        assert np.array_equal(got_depth, want_depth) and np.array_equal(got, want), (o0, d0)
    hand = dict(view, o=np.array([np.nextafter(16.0, 0.0), 8.25, 44.5]), dw=np.array([9e-17, 0.5, 0.0]), num_steps=60)
    assert V.cast_device(prepared, hand, 1, 1)[1][0, 0] == 10


def test_paint_tiles_guards_tiles_that_leave_the_canvas_and_bad_records():
    case = synthetic_case((30, 26, 22), (1.0, 1.0, 1.0), 5)
    dev = on_device(case)
    fill, line = V.colour_table(None, 0.45), V.colour_table(None, 1.0)

    def records(c):
        f32 = dict(kind="f32", volume=c["image"], channel=0, vmin=-50.0, vmax=150.0, shape=(30, 26, 22),
                   overlays=[(c["label"], fill, "fill"), (c["pred"], line, "outline")], origin=(0.5, 0.5), step=(1.0, 1.0))
        u8 = dict(kind="u8", volume=c["pred"], table=line, shape=(30, 26, 22), overlays=[(c["label"], line, "outline")],
                  origin=(0.25, 0.25), step=(0.5, 0.5))
        return [dict(f32, axis=0, index=15, x0=-5, y0=-7, w=22, h=26),            # leaves the canvas at the top left
                dict(f32, axis=2, index=11, x0=30, y0=30, w=26, h=30),            # and at the bottom right
                dict(u8, axis=1, index=13, x0=20, y0=0, w=44, h=28),              # ends beyond the right edge; 2 x zoom
                dict(f32, axis=1, index=26, x0=0, y0=30, w=22, h=30),             # index == extent: paints nothing
                dict(f32, axis=0, index=3, channel=1, x0=0, y0=30, w=22, h=26),   # no such channel: paints nothing
                dict(u8, axis=2, index=-1, x0=0, y0=30, w=26, h=30),              # negative index: paints nothing
                dict(f32, axis=1, index=2, x0=-4, y0=22, w=22, h=30)]             # a good one in what is left (disjoint)

    got = V.paint_tiles(records(dev), 52, 50)
    want = V.paint_tiles(records(case), 52, 50)
    assert got.shape == (52, 50, 3) and np.array_equal(got, want)
    assert want[:19, :17].any() and want[30:, 30:].any() and want[:28, 20:].any() and want[22:, :18].any()
    only_good = V.paint_tiles([r for i, r in enumerate(records(case)) if i not in (3, 4, 5)], 52, 50)
    assert np.array_equal(want, only_good)


def test_an_all_zero_mask_gives_background_and_a_plain_sheet():
    case = synthetic_case((40, 33, 21), (1.0, 1.0, 2.0), 3)
    case["pred"][:] = 0
    case["label"][:] = 0
    dev = on_device(case)
    pictures, depth = V.render_case(dev, views=((30, 20), (100, 0)), size=32, return_depth=True)
    assert pictures.shape == (2, 32, 32, 3) and not pictures.any() and np.all(depth == -1)
    sheet = V.case_sheet(dev, num_slices=3)
    assert np.array_equal(sheet, V.case_sheet(case, num_slices=3))
    assert np.array_equal(sheet[..., 0], sheet[..., 1]) and sheet.any()


def test_a_cascade_prediction_that_stays_in_hbm_is_previewed_without_a_host_copy(golden_dir, monkeypatch):
    z = np.load(os.path.join(golden_dir, "g9_cascade.npz"))
    coarse = network.ResUnet3D(num_pool=2, num_features=4, in_channels=1, out_channels=1)
    detail = network.ResUnet3D(num_pool=2, num_features=4, in_channels=1, out_channels=3)
    coarse.load_state_dict({k[len("coarse/w/"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("coarse/w/")})
    detail.load_state_dict({k[len("detail/w/"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("detail/w/")})
    stats = dict(zip(("mean", "std", "pct_00_5", "pct_99_5"), (float(v) for v in z["stats"])))
    case = {"case_id": "g9", "image": z["image"], "affine": z["affine"]}
    out = T.cascade_predict_case(case, coarse.to(DEV).eval(), tuple(z["params"][0]), stats,
                                 tuple(int(v) for v in z["patches"][0]), detail.to(DEV).eval(), tuple(z["params"][1]),
                                 stats, tuple(int(v) for v in z["patches"][1]), step_per_patch=int(z["scalars"][0]),
                                 region_threshold=int(z["scalars"][1]), crop_padding=int(z["scalars"][2]), verbose=False,
                                 on_device=True, return_device=True)
    assert torch.is_tensor(out["pred"]) and out["pred"].is_cuda and out["pred"].dtype == torch.uint8
    dev_case = {"pred": out["pred"], "affine": out["affine"]}
    if out.get("image") is not None:
        dev_case["image"] = out["image"]
    # nothing of the volume's size may be downloaded while the device route runs: only panels, pictures, brick grids
    volume_shapes = {tuple(out["pred"].shape)} | ({tuple(dev_case["image"].shape)} if "image" in dev_case else set())
    real_cpu, real_to, downloads = torch.Tensor.cpu, torch.Tensor.to, []

    def guarded_cpu(self, *args, **kwargs):
        if self.is_cuda:
            downloads.append(tuple(self.shape))
            assert tuple(self.shape) not in volume_shapes, "a volume of shape %s was downloaded" % (tuple(self.shape),)
        return real_cpu(self, *args, **kwargs)

    def guarded_to(self, *args, **kwargs):
        target = args[0] if args else kwargs.get("device")
        if self.is_cuda and (target == "cpu" or (isinstance(target, torch.device) and target.type == "cpu")):
            assert tuple(self.shape) not in volume_shapes, "a volume of shape %s was downloaded" % (tuple(self.shape),)
        return real_to(self, *args, **kwargs)

    monkeypatch.setattr(torch.Tensor, "cpu", guarded_cpu)
    monkeypatch.setattr(torch.Tensor, "to", guarded_to)
    picture = T.preview_case(dev_case, num_slices=4, size=64, views=((30, 20), (150, -10)))
    monkeypatch.undo()
    assert downloads and picture.shape[2] == 3
    host_case = {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in dev_case.items()}
    assert host_case["pred"].max() >= 1
    assert np.array_equal(picture, T.preview_case(host_case, num_slices=4, size=64, views=((30, 20), (150, -10))))
    assert picture[-64:].any()


def test_full_size_views_equal_the_numpy_route_on_a_sub_rectangle():
    shape, spacing = (512, 512, 256), (0.78, 0.78, 1.5)
    volume = torch.zeros(shape, dtype=torch.uint8, device=DEV)
    gx, gy, gz = (torch.arange(n, device=DEV, dtype=torch.float32) for n in shape)
    for label, (cx, cy, cz, r) in ((1, (300, 310, 170, 150)), (2, (340, 330, 190, 60)), (3, (440, 440, 250, 11))):
        d2 = ((gx - cx) * spacing[0])[:, None, None] ** 2 + ((gy - cy) * spacing[1])[None, :, None] ** 2 \
            + ((gz - cz) * spacing[2])[None, None, :] ** 2
        volume[d2 <= float(r * r) * spacing[0] ** 2] = label
    case = {"pred": volume, "affine": np.diag(list(spacing) + [1.0])}
    views = ((30, 20), (120, 20), (210, -20), (300, 60))
    got, got_depth = V.render_case(case, views=views, size=768, alpha={1: 0.35}, return_depth=True)
    assert (got_depth >= 0).any(axis=(1, 2)).all()
    host = volume.cpu().numpy()
    table = V.colour_table(None, {1: 0.35})
    box = V._brick_box(V._bricks_numpy(host, table), shape)
    assert box[1][0] == 456 and box[1][2] == 256           # the small ball near the far corner: element indices near 2^26
    for i in (0, 3):
        view = V.fit_view(box, spacing, views[i][0], views[i][1], 768)
        u0, v0, w, h = 350, 330, 72, 48
        want, want_depth = V.cast_numpy(host, table, view, h, w, u0, v0)
        assert (want_depth >= 0).any()
        assert np.array_equal(got_depth[i, v0:v0 + h, u0:u0 + w], want_depth)
        assert np.array_equal(got[i, v0:v0 + h, u0:u0 + w], want)
