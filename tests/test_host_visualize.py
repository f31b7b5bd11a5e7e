"""visualize / pngfile on the host: the reference's panels, the slice-tile and ray-cast contracts in numpy, a
pure-Python twin of the device kernel's word and brick arithmetic, PNG files and the preview drivers."""
import math
import os

import numpy as np
import pytest

import pngfile
import visualize as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ case_panels
def _small_case(channels):
    image = np.arange(4 * 6 * 5 * channels, dtype=np.float32).reshape(4, 6, 5, channels) * 0.5 - 7.0
    label = (np.arange(4 * 6 * 5).reshape(4, 6, 5) % 4).astype(np.uint8)
    pred = (np.arange(4 * 6 * 5).reshape(4, 6, 5) % 3).astype(np.uint8)
    return image, label, pred


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("have", [("label",), ("pred",), ("label", "pred")])
def test_case_panels_count_order_contents_and_ranges(channels, have):
    image, label, pred = _small_case(channels)
    case = {"image": image}
    case.update({k: {"label": label, "pred": pred}[k] for k in have})
    for axi, pct, index in ((0, 0.5, 2), (1, 0.5, 3), (2, 0.5, 2), (0, 0.625, 2), (0, 0.875, 4), (0, 0.375, 2),
                            (1, 0.25, 2), (1, 0.75, 4), (2, 0.3, 2), (2, 0.7, 4)):
        # round() is Python's: 4 * .625 = 2.5 -> 2, 4 * .875 = 3.5 -> 4 (= the extent: raises), 4 * .375 = 1.5 -> 2
        if index >= image.shape[axi]:
            with pytest.raises(IndexError):
                V.case_panels(case, pct, axi)
            continue
        panels, ranges = V.case_panels(case, pct, axi)
        cut = (lambda v: v[index]) if axi == 0 else (lambda v: v[:, index]) if axi == 1 else (lambda v: v[:, :, index])
        want = [cut(image[..., c]) for c in range(channels)] + [cut({"label": label, "pred": pred}[k]) for k in have]
        assert len(panels) == len(want) == len(ranges)
        for got, ref in zip(panels, want):
            assert got.dtype == ref.dtype and np.array_equal(got, ref)
        window = [np.percentile(image, 0.5), np.percentile(image, 99.5)]
        assert ranges[:channels] == [window] * channels
        assert ranges[channels:] == [[0, 3] if k == "label" else [0, 2] for k in have]


def test_case_panels_one_hot_counts_the_labels_channels_for_the_prediction():
    image, label, pred = _small_case(1)
    case = {"image": image, "label": np.eye(4, dtype=np.float32)[label], "pred": np.eye(5, dtype=np.float32)[pred]}
    panels, ranges = V.case_panels(case, 0.5, 2, one_hot_label=True, one_hot_pred=True)
    assert len(panels) == 1 + 4 + 4 and ranges[1:] == [[0, 1]] * 8
    assert np.array_equal(panels[1 + 2], case["label"][:, :, 2, 2]) and np.array_equal(panels[5 + 3], case["pred"][:, :, 2, 3])


def test_case_panels_match_the_reference_recording(golden_dir):
    g = np.load(os.path.join(golden_dir, "g11_visualize.npz"))
    for i, (pct, axi, hl, hp) in enumerate(g["calls"]):
        label, pred = g["label"], g["pred"]
        case = {"image": g["image"], "label": np.eye(4, dtype=np.float32)[label] if hl else label,
                "pred": np.eye(5, dtype=np.float32)[pred] if hp else pred}
        panels, ranges = V.case_panels(case, float(pct), int(axi), bool(hl), bool(hp))
        assert len(panels) == int(g["n_%d" % i])
        assert np.array_equal(np.array(ranges, dtype=np.float64), g["ranges_%d" % i])
        for j, panel in enumerate(panels):
            assert np.array_equal(panel, g["panel_%d_%d" % (i, j)])


def test_case_plt_draws_under_agg_and_imports_matplotlib_lazily():
    import subprocess
    import sys
    code = ("import sys; sys.path.insert(0, %r); import visualize; assert 'matplotlib' not in sys.modules; "
            "import matplotlib; matplotlib.use('Agg'); import numpy as np; "
            "visualize.case_plt({'image': np.zeros((4, 4, 4, 1), np.float32), 'label': np.ones((4, 4, 4), np.uint8)}); "
            "print('drawn')" % os.path.dirname(V.__file__))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "drawn" in out.stdout, out.stderr


# ------------------------------------------------------------------------------------------------ slice tiles
def _tile(volume, **kw):
    t = dict(kind="f32", volume=volume, channel=0, vmin=0.0, vmax=1.0, shape=volume.shape[:3], axis=0, index=0, x0=0, y0=0,
             w=volume.shape[2], h=volume.shape[1], origin=(0.5, 0.5), step=(1.0, 1.0), overlays=[])
    t.update(kw)
    return t


def test_tiles_window_and_nearest_voxel_sampling():
    image = np.zeros((1, 2, 3, 1), dtype=np.float32)
    image[0, :, :, 0] = [[-5.0, 0.0, 10.0], [20.0, 30.0, np.nan]]
    # 4 x 6 pixels over 2 x 3 voxels: step 0.5, sampled at pixel centres
    got = V.paint_tiles([_tile(image, vmin=0.0, vmax=20.0, w=6, h=4, origin=(0.25, 0.25), step=(0.5, 0.5))], 4, 6)
    grey = np.array([[0, 0, 128], [255, 255, 0]], dtype=np.uint8)              # floor(255 * 0.5 + 0.5) = 128; NaN -> 0
    assert np.array_equal(got[..., 0], np.repeat(np.repeat(grey, 2, axis=0), 2, axis=1))
    assert np.array_equal(got[..., 0], got[..., 1]) and np.array_equal(got[..., 0], got[..., 2])
    # pixels whose voxel lies outside are black; pixels outside the canvas are dropped
    got = V.paint_tiles([_tile(image, vmin=-10.0, vmax=0.0, w=4, h=3, x0=1, y0=-1)], 3, 4)
    assert np.array_equal(got[..., 0], [[0, 255, 255, 0], [0, 0, 0, 0], [0, 0, 0, 0]])


def test_tiles_fill_and_outline_of_a_two_voxel_cube():
    image = np.full((6, 6, 6, 1), 100.0, dtype=np.float32)
    cube = np.zeros((6, 6, 6), dtype=np.uint8)
    cube[2:4, 2:4, 2:4] = 1
    big = np.zeros((6, 6, 6), dtype=np.uint8)
    big[1:5, 1:5, 1:5] = 2
    fill = np.zeros((256, 4), dtype=np.uint8)
    fill[1] = (200, 0, 50, 128)
    line = np.zeros((256, 4), dtype=np.uint8)
    line[2] = (0, 255, 0, 255)
    t = _tile(image, vmin=0.0, vmax=200.0, axis=2, index=2, w=6, h=6, overlays=[(cube, fill, "fill"), (big, line, "outline")])
    got = V.paint_tiles([t], 6, 6)
    g = 128                                                                      # floor(255 * 0.5 + 0.5)
    want = np.full((6, 6, 3), g, dtype=np.uint8)
    want[2:4, 2:4] = [(128 * 200 + 127 * g + 127) // 255, (127 * g + 127) // 255, (128 * 50 + 127 * g + 127) // 255]
    ring = np.zeros((6, 6), dtype=bool)
    ring[1:5, 1:5] = True
    ring[2:4, 2:4] = False                                                       # 4 x 4 square: its 12 border voxels
    want[ring] = (0, 255, 0)
    assert np.array_equal(got, want)
    assert tuple(want[2, 2]) == (164, 64, 89)
    # a slice beside the cube: no fill; a structure that touches the border is closed there (outside reads 0)
    edge = np.zeros((6, 6, 6), dtype=np.uint8)
    edge[0:2, :, :] = 2
    got = V.paint_tiles([_tile(image, vmin=0.0, vmax=200.0, axis=2, index=0, w=6, h=6, overlays=[(cube, fill, "fill"),
                                                                                                (edge, line, "outline")])], 6, 6)
    assert np.all(got[0, :, 1] == 255) and np.all(got[1, :, 1] == 255) and np.all(got[2:, :, 1] == g)
    # a uint8 volume shown through its table
    got = V.paint_tiles([_tile(big, kind="u8", table=line, axis=0, index=1, w=6, h=6, overlays=[])], 6, 6)
    assert np.array_equal(got[..., 1], np.where(big[1] == 2, 255, 0))


def test_case_sheet_layout_square_pixels_and_slices_over_the_overlays():
    rng = np.random.default_rng(0)
    image = rng.normal(size=(24, 20, 10, 1)).astype(np.float32)
    label = np.zeros((24, 20, 10), dtype=np.uint8)
    label[9:15, 4:12, 2:7] = 1
    case = {"image": image, "label": label, "pred": label.copy(), "affine": np.diag([1.0, 1.0, 3.0, 1.0])}
    sheet = V.case_sheet(case, num_slices=4, pixel_mm=1.0)
    # rows: axis 0 tiles 20 x 30, axis 1 tiles 24 x 30, axis 2 tiles 24 x 20; 2 pixels between tiles and rows
    assert sheet.shape == (20 + 2 + 24 + 2 + 24, 4 * 30 + 3 * 2, 3) and sheet.dtype == np.uint8
    # axis 0 slices are centred in four equal parts of the brick box 8 .. 16: x = 9, 11, 13 cut the label, x = 15 does not
    row = V.case_sheet(case, axes=(0,), num_slices=4, pixel_mm=1.0)
    coloured = row[..., 0].astype(int) != row[..., 2]
    assert [bool(coloured[:, 32 * k:32 * k + 30].any()) for k in range(4)] == [True, True, True, False]
    assert np.array_equal(V.case_sheet({"pred": label}, axes=(2,), num_slices=2, pixel_mm=1.0)[..., 0] != 0,
                          np.concatenate([label[:, :, 2] != 0, np.zeros((24, 2), bool), label[:, :, 6] != 0], axis=1))


# ------------------------------------------------------------------------------------------------ ray cast
def _sphere(shape, centre, radius, spacing=(1.0, 1.0, 1.0)):
    grid = np.indices(shape).astype(np.float64)
    d2 = sum(((grid[c] + 0.5) * spacing[c] - centre[c]) ** 2 for c in range(3))
    return d2 <= radius * radius


def test_axis_aligned_view_of_a_box_has_the_depth_and_shade_computed_by_hand():
    volume = np.zeros((24, 24, 24), dtype=np.uint8)
    volume[8:16, 8:16, 8:16] = 1
    table = V.colour_table({1: (200, 100, 50)})
    view = V.fit_view(([8, 8, 8], [16, 16, 16]), (1.0, 1.0, 1.0), 0, 0, 32)
    assert np.allclose(view["dw"], [-0.5, 0, 0]) and view["num_steps"] == 19      # camera on +x, looking along -x
    rgb, depth = V.cast_numpy(volume, table, view, 32, 32)
    hit = depth >= 0
    # samples start half a voxel in front of the face x = 16 and advance by half a voxel: the first one inside is n = 2
    # (n = 1 sits on the face itself, floor(16.0) = 16, outside the box)
    assert set(np.unique(depth)) == {-1, 2}
    side = 8 / (8 * 1.04 / 32)
    assert abs(math.sqrt(hit.sum()) - side) <= 1.0
    inner = depth[12:20, 12:20]
    assert np.all(inner == 2)
    shade = view["ambient"] + view["diffuse"] * view["light"][0]                   # the face's normal is +x
    want = [int(math.floor(shade * c + 0.5)) for c in (200, 100, 50)]
    assert np.all(rgb[12:20, 12:20] == want)
    assert np.all(rgb[~hit] == 0)


def test_sphere_depth_is_symmetric_and_its_silhouette_has_the_area_of_a_disc():
    volume = _sphere((40, 40, 40), (20.0, 20.0, 20.0), 12.0).astype(np.uint8)
    view = V.fit_view(([0, 0, 0], [40, 40, 40]), (1.0, 1.0, 1.0), 90, 0, 80)
    rgb, depth = V.cast_numpy(volume, V.colour_table(), view, 80, 80)
    assert np.array_equal(depth, depth[::-1]) and np.array_equal(depth, depth[:, ::-1])
    pixel = 40 * 1.04 / 80
    r = 12.0 / pixel
    area = (depth >= 0).sum()
    assert math.pi * (r - 1) ** 2 <= area <= math.pi * (r + 1) ** 2
    assert rgb[40, 40].max() > rgb[40, 40 + int(r) - 2].max() > 0                 # lit centre, darker limb


def test_a_box_inside_a_box_shows_only_through_a_translucent_wall_and_an_empty_selection_is_background():
    volume = np.zeros((32, 32, 32), dtype=np.uint8)
    volume[4:28, 4:28, 4:28] = 1
    alone = volume.copy()
    volume[12:20, 12:20, 12:20] = 2
    case, hollow = {"pred": volume}, {"pred": alone}
    opaque = V.render_case(case, views=((0, 0),), size=48)
    assert np.array_equal(opaque, V.render_case(hollow, views=((0, 0),), size=48))
    glass, depth = V.render_case(case, views=((0, 0),), size=48, alpha={1: 0.35}, return_depth=True)
    empty = V.render_case(hollow, views=((0, 0),), size=48, alpha={1: 0.35})
    changed = (glass != empty).any(axis=-1)[0]
    inner = V.render_case(case, labels=(2,), views=((0, 0),), size=48, return_depth=True)[1][0] >= 0
    # the view boxes differ (fitted to the drawn labels), so project the inner box by hand: 8 voxels of the
    # 32 of the outer box's bricks, centred
    rows, cols = np.nonzero(changed)
    assert changed.sum() > 0 and rows.min() == cols.min() and rows.max() == cols.max()
    assert abs((rows.max() - rows.min() + 1) - 8 / (32 * 1.04 / 48)) <= 1.0 and changed[rows.min():rows.max() + 1,
                                                                                      cols.min():cols.max() + 1].all()
    assert inner.sum() > 0 and (depth >= 0).sum() > changed.sum()
    nothing, depth = V.render_case(case, labels=(7,), views=((10, 20), (200, -30)), size=16, return_depth=True)
    assert nothing.shape == (2, 16, 16, 3) and not nothing.any() and np.all(depth == -1)


# ------------------------------------------------------------------------------------------------ the kernel's twin
def _twin_cast(volume, table, view, H, W):
    """csrc/render.hip's rd_prepare_kernel and rd_surface_kernel restated ray by ray in Python: packed 64-voxel words,
    8 x 8 x 8 brick bytes, the slab clip and the jumps over empty bricks."""
    X, Y, Z = volume.shape
    ext = (X, Y, Z)
    words = -(-Z // 64)
    drawn = table[:, 3] != 0
    drawn[0] = False
    mask = [[[0] * words for _ in range(Y)] for _ in range(X)]
    bricks = np.zeros((-(-X // 8), -(-Y // 8), 8 * words), dtype=np.uint8)
    for x in range(X):
        for y in range(Y):
            for w in range(words):
                word = 0
                for b in range(min(64, Z - 64 * w)):
                    word |= int(drawn[volume[x, y, 64 * w + b]]) << b
                mask[x][y][w] = word
                for q in range(8):
                    if (word >> (8 * q)) & 0xff:
                        bricks[x // 8, y // 8, 8 * w + q] = 1
    rgb = np.zeros((H, W, 3), dtype=np.uint8)
    depth = np.full((H, W), -1, dtype=np.int32)
    o, du, dv, dw = (np.asarray(view[k], dtype=np.float64) for k in ("o", "du", "dv", "dw"))
    steps = int(view["num_steps"])
    visited = 0
    for v in range(H):
        for u in range(W):
            base = [(o[c] + np.float64(u) * du[c]) + np.float64(v) * dv[c] for c in range(3)]
            tmin, tmax = 0.0, float(steps)
            for c in range(3):
                if dw[c] == 0.0:
                    if not (base[c] >= 0.0 and base[c] < ext[c]):
                        tmax = -1.0
                else:
                    t0, t1 = (0.0 - base[c]) / dw[c], (ext[c] - base[c]) / dw[c]
                    tmin, tmax = max(tmin, min(t0, t1)), min(tmax, max(t0, t1))
            n, n_hi = 0, 0
            if tmax >= tmin:
                n, n_hi = int(max(0.0, math.floor(tmin) - 2.0)), int(min(float(steps), math.ceil(tmax) + 3.0))
            T, C, first, prev = np.float64(1.0), [np.float64(0.0)] * 3, -1, 0
            while n < n_hi:
                visited += 1
                q = [base[c] + np.float64(n) * dw[c] for c in range(3)]
                f = [math.floor(x) for x in q]
                if not all(0 <= f[c] < ext[c] for c in range(3)):
                    prev, n = 0, n + 1
                    continue
                b = [f[0] >> 3, f[1] >> 3, f[2] >> 3]
                if not bricks[b[0], b[1], b[2]]:
                    t = 1048576.0
                    for c in range(3):
                        if dw[c] > 0.0:
                            t = min(t, (float(b[c] * 8 + 8) - q[c]) / dw[c])
                        elif dw[c] < 0.0:
                            t = min(t, (float(b[c] * 8) - q[c]) / dw[c])
                    jump = int(math.floor(t)) - 1                      # an estimate; accepted only if the last sample
                    if jump > 1:                                       # passed over lies in this brick by the contract
                        e = [base[c] + np.float64(n + jump - 1) * dw[c] for c in range(3)]
                        if not all(b[c] * 8 <= e[c] < b[c] * 8 + 8 for c in range(3)):
                            jump = 1
                    prev, n = 0, n + max(1, jump)
                    continue
                if not (mask[f[0]][f[1]][f[2] >> 6] >> (f[2] & 63)) & 1:
                    prev, n = 0, n + 1
                    continue
                L = int(volume[f[0], f[1], f[2]])
                if L != prev:
                    g = [0, 0, 0]
                    for dx in (-1, 0, 1):
                        for dy in (-1, 0, 1):
                            for dz in (-1, 0, 1):
                                i, j, k = f[0] + dx, f[1] + dy, f[2] + dz
                                if 0 <= i < X and 0 <= j < Y and 0 <= k < Z and volume[i, j, k] == L:
                                    g[0] += dx
                                    g[1] += dy
                                    g[2] += dz
                    m = [np.float64(-g[c]) / view["spacing"][c] for c in range(3)]
                    light = view["light"]
                    dot = (m[0] * light[0] + m[1] * light[1]) + m[2] * light[2]
                    len2 = (m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]
                    shade = view["ambient"] + view["diffuse"] if len2 == 0 else \
                        view["ambient"] + (view["diffuse"] * max(dot, 0.0)) / np.sqrt(len2)
                    a = np.float64(table[L, 3]) / 255.0
                    k = (T * a) * shade
                    C = [C[c] + k * np.float64(table[L, c]) for c in range(3)]
                    T = T * (1.0 - a)
                    first = n if first < 0 else first
                    if T < 0.00390625:
                        break
                prev, n = L, n + 1
            for c in range(3):
                x = C[c] + T * view["background"][c]
                rgb[v, u, c] = int(math.floor(min(max(x, 0.0), 255.0) + 0.5))
            depth[v, u] = first
    return rgb, depth, visited


@pytest.mark.parametrize("seed,shape,spacing", [(1, (21, 17, 70), (0.8, 0.8, 2.5)), (2, (9, 30, 13), (1.5, 0.7, 1.0)),
                                                (3, (16, 16, 64), (1.0, 1.0, 1.0))])
def test_twin_of_the_kernels_word_and_brick_arithmetic_draws_the_definitions_picture(seed, shape, spacing):
    rng = np.random.default_rng(seed)
    volume = np.zeros(shape, dtype=np.uint8)
    centre = [shape[c] * spacing[c] * f for c, f in zip(range(3), (0.45, 0.55, 0.5))]
    reach = min(shape[c] * spacing[c] for c in range(3))
    volume[_sphere(shape, centre, 0.42 * reach, spacing)] = 1
    volume[_sphere(shape, centre, 0.2 * reach, spacing)] = 2
    volume[_sphere(shape, [centre[0], centre[1], centre[2] * 1.5], 0.12 * reach, spacing)] = 3
    volume[rng.random(shape) < 0.003] = 4                                  # speckle: isolated voxels, zero normals
    volume[rng.random(shape) < 0.003] = 9                                  # a label the table does not draw
    table = V.colour_table(None, {1: 0.35, 3: 0.6}, labels=(1, 2, 3, 4))
    box = V._brick_box(V._bricks_numpy(volume, table), shape)
    size = 20
    for azimuth, elevation in ((0, 0), (37, 23), (250, -61), (90, 90)):
        view = V.fit_view(box, spacing, azimuth, elevation, size, background=(10, 20, 30))
        rgb, depth = V.cast_numpy(volume, table, view, size, size)
        twin_rgb, twin_depth, visited = _twin_cast(volume, table, view, size, size)
        assert np.array_equal(depth, twin_depth) and np.array_equal(rgb, twin_rgb)
        assert (depth >= 0).any() and visited < size * size * view["num_steps"]


def test_a_view_whose_box_is_mostly_empty_is_crossed_in_jumps():
    volume = np.zeros((64, 64, 64), dtype=np.uint8)
    volume[40:44, 40:44, 40:44] = 1
    table = V.colour_table()
    view = V.fit_view(([0, 0, 0], [64, 64, 64]), (1.0, 1.0, 1.0), 30, 20, 12)
    rgb, depth = V.cast_numpy(volume, table, view, 12, 12)
    twin_rgb, twin_depth, visited = _twin_cast(volume, table, view, 12, 12)
    assert np.array_equal(rgb, twin_rgb) and np.array_equal(depth, twin_depth) and (depth >= 0).any()
    assert visited * 3 < 12 * 12 * view["num_steps"]


def _plates_behind_brick_faces():
    """A brick-aligned box (two voxels at its corners) with thin plates just behind the brick faces x = 16, y = 16 and
    z = 64: a ray that runs along such a face and drifts across it by rounding alone meets them."""
    volume = np.zeros((32, 32, 96), dtype=np.uint8)
    volume[16, 13:15, 40:48] = 1
    volume[16, 17:19, 40:48] = 2
    volume[10:13, 16, 50:56] = 3
    volume[19:22, 15, 50:56] = 1
    volume[10:12, 20:22, 64] = 2
    volume[20:22, 10:12, 63] = 3
    volume[8, 8, 32] = 1
    volume[23, 23, 71] = 1
    return volume


@pytest.mark.parametrize("size", [15, 33, 65, 16])
def test_views_along_the_axes_whose_direction_has_components_below_an_ulp_of_the_coordinates(size):
    # cos(270 deg) = -1.8e-16, sin(180 deg) = 1.2e-16: dw has a component far below one ulp of a coordinate, and on a
    # brick-aligned box with an odd picture size the middle column starts one ulp from a brick face, so the rounded
    # positions of the contract cross the face at another sample than the real line does
    volume = _plates_behind_brick_faces()
    table = V.colour_table(None, {1: 0.5})
    box = V._brick_box(V._bricks_numpy(volume, table), volume.shape)
    assert box == ([8, 8, 32], [24, 24, 72])
    for spacing in ((1.0, 1.0, 1.0), (0.75, 0.75, 3.0)):
        for azimuth, elevation in ((270, 0), (90, 0), (180, 0), (0, 0), (0, 90), (0, -90), (270, 90), (180, -90)):
            view = V.fit_view(box, spacing, azimuth, elevation, size)
            rgb, depth = V.cast_numpy(volume, table, view, size, size)
            twin_rgb, twin_depth, _ = _twin_cast(volume, table, view, size, size)
            assert np.array_equal(depth, twin_depth) and np.array_equal(rgb, twin_rgb), (spacing, azimuth, elevation)
            assert (depth >= 0).any()


def test_a_ray_that_rounding_alone_carries_across_a_brick_face_still_meets_the_surface_behind_it():
    volume = np.zeros((32, 32, 32), dtype=np.uint8)
    volume[16, 13:15, 16] = 1                                  # in the brick next to the one the ray starts in
    table = V.colour_table()
    view = V.fit_view(([8, 8, 8], [24, 24, 24]), (1.0, 1.0, 1.0), 270, 0, 1)
    for o0, d0 in ((np.nextafter(16.0, 0.0), 9e-17), (np.nextafter(16.0, 0.0), 3e-16), (16.0, -9e-17), (np.nextafter(16.0, 32.0), -4e-16)):
        hand = dict(view, o=np.array([o0, 8.25, 16.5]), dw=np.array([d0, 0.5, 0.0]), num_steps=60)
        rgb, depth = V.cast_numpy(volume, table, hand, 1, 1)
        twin_rgb, twin_depth, _ = _twin_cast(volume, table, hand, 1, 1)
        assert np.array_equal(depth, twin_depth) and np.array_equal(rgb, twin_rgb), (o0, d0)
    hand = dict(view, o=np.array([np.nextafter(16.0, 0.0), 8.25, 16.5]), dw=np.array([9e-17, 0.5, 0.0]), num_steps=60)
    assert V.cast_numpy(volume, table, hand, 1, 1)[1][0, 0] == 10      # x reaches 16.0 by rounding at n = 10 (y = 13.25)


# ------------------------------------------------------------------------------------------------ PNG
@pytest.mark.parametrize("shape", [(1, 1, 3), (7, 5, 3), (16, 33, 3), (3, 9), (1, 1), (20, 17)])
def test_png_round_trip(tmp_path, shape):
    rng = np.random.default_rng(sum(shape))
    picture = rng.integers(0, 256, size=shape, dtype=np.uint8)
    path = tmp_path / "p.png"
    pngfile.write_png(path, picture)
    back = pngfile.read_png(path)
    assert back.dtype == np.uint8 and np.array_equal(back, picture)
    data = bytearray(path.read_bytes())
    data[-20] ^= 0x01                                                         # inside the IDAT chunk
    (tmp_path / "bad.png").write_bytes(bytes(data))
    with pytest.raises(ValueError, match="CRC"):
        pngfile.read_png(tmp_path / "bad.png")
    with pytest.raises(ValueError):
        pngfile.write_png(path, picture.astype(np.float32))


def test_png_is_read_by_a_foreign_reader_and_reads_a_foreign_writers_filters(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(5)
    for shape in ((13, 11, 3), (6, 7)):
        picture = rng.integers(0, 256, size=shape, dtype=np.uint8)
        picture[2:5] = np.arange(shape[1], dtype=np.uint8).reshape((-1,) + (1,) * (len(shape) - 2))  # smooth rows: filters
        pngfile.write_png(tmp_path / "ours.png", picture)
        assert np.array_equal(np.asarray(Image.open(tmp_path / "ours.png")), picture)
        Image.fromarray(picture).save(tmp_path / "theirs.png", optimize=True)
        assert np.array_equal(pngfile.read_png(tmp_path / "theirs.png"), picture)


# ------------------------------------------------------------------------------------------------ drivers
def test_batch_preview_writes_one_png_per_case(tmp_path):
    import nifti
    import trainer
    affine = np.diag([1.0, 1.0, 2.0, 1.0])
    rng = np.random.default_rng(3)
    for d in ("pred", "image", "label"):
        (tmp_path / d).mkdir()
    for i in range(2):
        pred = np.zeros((20, 16, 10), dtype=np.uint8)
        pred[5 + i:14, 4:12, 2:8] = 1
        pred[8:11, 6:9, 4:6] = 2
        nifti.save(pred, affine, tmp_path / "pred" / ("case_%d.pred.nii.gz" % i))
        nifti.save(np.roll(pred, 1, axis=1), affine, tmp_path / "label" / ("case_%d.nii.gz" % i))
        nifti.save(rng.normal(size=pred.shape).astype(np.float32), affine, tmp_path / "image" / ("case_%d.nii.gz" % i))
    pictures = trainer.batch_preview(tmp_path / "pred", tmp_path / "out", tmp_path / "image", tmp_path / "label",
                                     num_slices=3, size=40, pixel_mm=1.0, views=((30, 20), (200, 10)))
    files = sorted(p.name for p in (tmp_path / "out").iterdir())
    assert files == ["case_0.preview.png", "case_1.preview.png"]
    # rows of 16 x 20, 20 x 20 and 20 x 16 tiles, then the two 40 x 40 views
    assert pictures[0].shape == (16 + 2 + 20 + 2 + 20 + 2 + 40, max(3 * 20 + 4, 82), 3)
    for name, picture in zip(files, pictures):
        assert np.array_equal(pngfile.read_png(tmp_path / "out" / name), picture) and picture[-40:].any()
    alone = trainer.preview(tmp_path / "pred" / "case_0.pred.nii.gz", num_slices=3, size=40, pixel_mm=1.0, views=())
    assert alone.shape == (16 + 2 + 20 + 2 + 20, 64, 3) and alone.any()


def test_the_library_declares_the_render_entry_points_and_the_isa_check_lists_the_file():
    import _native as N
    for name in ("ru3d_render_tiles", "ru3d_render_surface_workspace_bytes", "ru3d_render_surface_prepare",
                 "ru3d_render_surface"):
        assert name in N.SIGNATURES, name
    assert N.lib.ru3d_version() == 201
    assert N.lib.ru3d_render_surface_workspace_bytes(512, 512, 256) == 512 * 512 * 4 * 8 + 64 * 64 * 32
    assert N.lib.ru3d_render_surface_workspace_bytes(2048, 2048, 512) == 0          # 2^31 voxels
    assert N.lib.ru3d_render_tiles(None, 1, None, 4, 4, None) < 0 and b"render_tiles" in N.lib.ru3d_last_error()
    assert '"render.hip"' in open(os.path.join(ROOT, "tools", "isa_check.py")).read()
    rows = [l.split() for l in open(os.path.join(ROOT, "profiles", "render_isa_check.txt")) if l.startswith("render.hip")]
    assert {r[1] for r in rows} == {"rd_tiles_kernel", "rd_prepare_kernel", "rd_surface_kernel"}
    assert all(int(r[5]) == 0 and int(r[6]) == 0 for r in rows)                     # no spills, no scratch
