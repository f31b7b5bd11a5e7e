"""Looking at a case: the reference's `grid_plt` / `case_plt` (visualize.py there), and pictures rendered without
matplotlib - a montage of slices with the label and the prediction drawn over the image (`case_sheet`) and shaded views
of the label volume (`render_case`) - as uint8 RGB arrays that `pngfile.write_png` stores.

Every function takes numpy arrays or HIP tensors.  numpy operands take the numpy route, which restates the contract of
include/ru3d.h ("rendering") in vectorised numpy; HIP tensors - what `cascade_predict_case(..., return_device=True)`
returns goes in as it is - take the device route (csrc/render.hip, and the order statistics of csrc/prepare.hip for
the percentiles): slices are cut, windows taken and pictures painted in HBM, and what crosses PCIe is the 2-D panels,
the range numbers and the finished canvases.  Both routes return the same arrays and the same numbers (`==`).
matplotlib is imported inside `grid_plt` only.
"""
import ctypes
import math

import numpy as np

BRICK = 8                                    # RD_BRICK of csrc/render.hip
PALETTE = ((230, 110, 80), (250, 220, 60), (80, 140, 250), (90, 220, 120), (200, 100, 230), (70, 210, 220),
           (240, 160, 60), (170, 170, 170))   # labels 1, 2, 3 ... (cyclic)


# ----------------------------------------------------------------------------------------------- operands
def _is_tensor(v):
    return type(v).__module__.startswith('torch') and hasattr(v, 'is_cuda')


def _is_hip(v):
    return _is_tensor(v) and v.is_cuda


def _host(v):
    """numpy view of a numpy array or a CPU tensor."""
    return v.numpy() if _is_tensor(v) else np.asarray(v)


def _device_of(*operands):
    for v in operands:
        if _is_hip(v):
            return v.device
    return None


def _to_device(v, device, dtype):
    """Contiguous HIP tensor of `dtype` ('f32' or 'u8'; integer volumes are clipped to 0 .. 255) on `device`."""
    import torch
    if not _is_tensor(v):
        v = np.asarray(v)
        v = v.astype(np.float32) if dtype == 'f32' else (v if v.dtype == np.uint8 else np.clip(v, 0, 255).astype(np.uint8))
        return torch.from_numpy(np.ascontiguousarray(v)).to(device)
    v = v.to(device)
    if dtype == 'f32':
        return v.to(torch.float32).contiguous()
    return (v if v.dtype == torch.uint8 else v.clamp(0, 255).to(torch.uint8)).contiguous()


def _to_host(v, dtype):
    v = _host(v.cpu() if _is_hip(v) else v)
    if dtype == 'f32':
        return np.ascontiguousarray(v, dtype=np.float32)
    return np.ascontiguousarray(v if v.dtype == np.uint8 else np.clip(v, 0, 255).astype(np.uint8))


def spacing_of(case):
    """Voxel size in millimetres per axis from the case's affine (column norms); ones without an affine."""
    affine = case.get('affine')
    if affine is None:
        return np.ones(3)
    a = np.asarray(affine, dtype=np.float64)
    s = np.sqrt((a[:3, :3] ** 2).sum(axis=0))
    if not np.all(np.isfinite(s)) or np.any(s <= 0):
        raise ValueError("affine: the voxel sizes %s are not positive" % (s,))
    return s


# ----------------------------------------------------------------------------------------------- the reference's two
def grid_plt(grid_list, value_ranges=None):
    """Show a figure with one row of panels per entry of grid_list, four inches a panel, axes hidden; column j is drawn
    with the colour limits value_ranges[j] = (vmin, vmax), or with matplotlib's own limits when no ranges are given."""
    import matplotlib.pyplot as plt
    columns = len(grid_list[0])
    limits = value_ranges if value_ranges else [(None, None)] * columns
    figure, axes = plt.subplots(len(grid_list), columns, figsize=(4 * columns, 4 * len(grid_list)), squeeze=False)
    for axes_row, panels in zip(axes, grid_list):
        for axis, panel, (low, high) in zip(axes_row, panels, limits):
            axis.imshow(panel, vmin=low, vmax=high)
            axis.set_axis_off()
    figure.tight_layout()
    plt.show()


def _percentiles(v, qs):
    """np.percentile(v, q) for q in qs.  A HIP tensor: two order statistics per percentile selected on the device
    (ru3d_order_stats), interpolated on the host with numpy's own expression."""
    if not _is_hip(v):
        return [np.percentile(_host(v), q) for q in qs]
    import torch
    import prepare
    flat = v.to(torch.float32).reshape(-1)
    plans = [prepare._quantile_plan(flat.numel(), q) for q in qs]
    ranks = sorted({r for lo, hi, _ in plans for r in (lo, hi)})
    picked = dict(zip(ranks, prepare.order_statistics(flat, ranks)))
    return [prepare._lerp(picked[lo], picked[hi], t) for lo, hi, t in plans]


def _cut(v, axi, index, channel=None):
    """v[index, :, :] (axi 0), v[:, index, :] (1) or v[:, :, index] (anything else), with the channel last when given;
    a HIP tensor is cut on the device and only the panel is downloaded."""
    if index >= v.shape[axi if axi in (0, 1) else 2]:
        raise IndexError("index %d is out of bounds for axis %d with size %d"
                         % (index, axi if axi in (0, 1) else 2, v.shape[axi if axi in (0, 1) else 2]))
    key = (index,) if axi == 0 else (slice(None), index) if axi == 1 else (slice(None), slice(None), index)
    if channel is not None:
        key = key + (slice(None),) * (3 - len(key)) + (channel,)
    panel = v[key]
    return panel.cpu().numpy() if _is_hip(panel) else (_host(panel) if _is_tensor(panel) else panel)


def _min_max(v):
    if _is_hip(v):
        return [v.min().cpu().numpy()[()], v.max().cpu().numpy()[()]]
    v = _host(v)
    return [v.min(), v.max()]


def case_panels(case, slice_pct=0.5, axi=0, one_hot_label=False, one_hot_pred=False):
    """(panels, value_ranges) of case_plt: one panel per image channel with the 0.5 / 99.5 percentiles of the whole
    image array, then the label and the prediction with their [min, max] - or, one-hot, one panel per channel with
    [0, 1]; the one-hot prediction loop counts label.shape[-1] channels, as the reference's does."""
    image = case['image']
    label = case['label'] if 'label' in case else None
    pred = case['pred'] if 'pred' in case else None
    index = round(image.shape[axi] * slice_pct)
    panels, ranges = [], []
    window = None
    for c in range(image.shape[-1]):
        panels.append(_cut(image, axi, index, c))
        if window is None:
            window = _percentiles(image, (0.5, 99.5))
        ranges.append(list(window))
    for volume, one_hot in ((label, one_hot_label), (pred, one_hot_pred)):
        if volume is None:
            continue
        if one_hot:
            for c in range(label.shape[-1]):
                panels.append(_cut(volume, axi, index, c))
                ranges.append([0, 1])
        else:
            panels.append(_cut(volume, axi, index))
            ranges.append(_min_max(volume))
    return panels, ranges


def case_plt(case, slice_pct=0.5, axi=0, one_hot_label=False, one_hot_pred=False):
    panels, ranges = case_panels(case, slice_pct, axi, one_hot_label, one_hot_pred)
    grid_plt([panels], value_ranges=ranges)


# ----------------------------------------------------------------------------------------------- colour tables
def colour_table(colours=None, alpha=1.0, labels=None):
    """uint8 [256, 4] RGBA rows: label l gets PALETTE[(l - 1) % 8] or colours[l]; its alpha byte is round(255 * alpha)
    (alpha: one number or {label: number}, missing labels opaque) for the labels in `labels` (None: 1 .. 255) and 0
    for every other label.  Label 0 is never drawn."""
    table = np.zeros((256, 4), dtype=np.uint8)
    drawn = range(1, 256) if labels is None else [int(l) for l in labels]
    for l in drawn:
        if not 1 <= l <= 255:
            raise ValueError("colour_table: label %r (1 .. 255)" % (l,))
        rgb = (colours or {}).get(l, PALETTE[(l - 1) % len(PALETTE)])
        a = alpha.get(l, 1.0) if isinstance(alpha, dict) else (1.0 if alpha is None else alpha)
        if not 0.0 <= float(a) <= 1.0:
            raise ValueError("colour_table: alpha %r of label %d (0 .. 1)" % (a, l))
        table[l] = (int(rgb[0]), int(rgb[1]), int(rgb[2]), int(round(255 * float(a))))
    return table


def _bricks_numpy(volume, table):
    """bool [BX, BY, BZ]: the 8 x 8 x 8 bricks of a uint8 volume that hold a drawn voxel (BZ = 8 ceil(Z / 64): a packed
    word of the device route is eight bricks long)."""
    drawn = table[:, 3] != 0
    drawn[0] = False
    m = drawn[volume]
    X, Y, Z = volume.shape
    bx, by, bz = -(-X // BRICK), -(-Y // BRICK), 8 * (-(-Z // 64))
    padded = np.zeros((bx * BRICK, by * BRICK, bz * BRICK), dtype=bool)
    padded[:X, :Y, :Z] = m
    return padded.reshape(bx, BRICK, by, BRICK, bz, BRICK).any(axis=(1, 3, 5))


class _Prepared:
    """The workspace of ru3d_render_surface_prepare for one (HIP volume, table) pair, and its brick grid on the host."""

    def __init__(self, volume, table):
        import torch
        import _native as N
        from _native import check, ptr, stream
        self.volume = volume
        self.table = torch.from_numpy(np.ascontiguousarray(table)).to(volume.device)
        X, Y, Z = volume.shape
        if X * Y * Z >= 1 << 31:
            raise ValueError("a %dx%dx%d volume has 2**31 voxels or more" % (X, Y, Z))
        self.ws = torch.empty(N.lib.ru3d_render_surface_workspace_bytes(X, Y, Z), dtype=torch.uint8, device=volume.device)
        N.note_device(volume.device)
        check(N.lib.ru3d_render_surface_prepare(ptr(volume), X, Y, Z, ptr(self.table), ptr(self.ws), self.ws.numel(),
                                                stream()), "render_surface_prepare")
        words = -(-Z // 64)
        shape = (-(-X // BRICK), -(-Y // BRICK), 8 * words)
        mask_bytes = -(-(X * Y * words * 8) // 256) * 256
        count = shape[0] * shape[1] * shape[2]
        self.bricks = self.ws[mask_bytes:mask_bytes + count].cpu().numpy().reshape(shape) != 0


def _brick_box(bricks, shape):
    """(lo [3], hi [3]) in voxels, hi exclusive: the bounding box of the set bricks clipped to the volume; None if empty."""
    if not bricks.any():
        return None
    lo, hi = [], []
    for axis in range(3):
        hit = np.nonzero(bricks.any(axis=tuple(a for a in range(3) if a != axis)))[0]
        lo.append(int(hit[0]) * BRICK)
        hi.append(min((int(hit[-1]) + 1) * BRICK, int(shape[axis])))
    return lo, hi


# ----------------------------------------------------------------------------------------------- slice sheets
def _in_plane(axis):
    return (1 if axis == 0 else 0), (1 if axis == 2 else 2)


def _paint_tile_numpy(canvas, t):
    """One tile record painted into the canvas with the contract's arithmetic."""
    H, W = canvas.shape[:2]
    shape = t['shape']
    if t['axis'] not in (0, 1, 2) or not 0 <= t['index'] < shape[t['axis']] or t['w'] < 1 or t['h'] < 1 or \
            (t['kind'] == 'f32' and not 0 <= t['channel'] < t['volume'].shape[3]):
        return                                                  # a bad record paints nothing
    ax_a, ax_b = _in_plane(t['axis'])
    fa = np.floor(t['origin'][0] + np.arange(t['h'], dtype=np.float64) * t['step'][0])
    fb = np.floor(t['origin'][1] + np.arange(t['w'], dtype=np.float64) * t['step'][1])
    ok = ((fa >= 0) & (fa < shape[ax_a]))[:, None] & ((fb >= 0) & (fb < shape[ax_b]))[None, :]
    a = np.where((fa >= 0) & (fa < shape[ax_a]), fa, 0).astype(np.int64)[:, None]
    b = np.where((fb >= 0) & (fb < shape[ax_b]), fb, 0).astype(np.int64)[None, :]
    if t['kind'] == 'f32':
        plane = np.take(t['volume'][..., t['channel']], t['index'], axis=t['axis'])
        val = plane[a, b].astype(np.float64)
        with np.errstate(all='ignore'):
            s = (val - t['vmin']) / (np.float64(t['vmax']) - np.float64(t['vmin']))
        s = np.where(s > 0, s, 0.0)
        s = np.where(s > 1, 1.0, s)
        grey = np.floor(255.0 * s + 0.5).astype(np.int64)
        rgb = np.stack([grey, grey, grey], axis=-1)
    else:
        plane = np.take(t['volume'], t['index'], axis=t['axis'])
        rgb = t['table'][plane[a, b], :3].astype(np.int64)
    for volume, table, mode in t['overlays']:
        plane = np.take(volume, t['index'], axis=t['axis'])
        l = plane[a, b]
        rgba = table[l].astype(np.int64)
        draw = rgba[..., 3] != 0
        if mode == 'outline':
            padded = np.pad(plane, 1)
            edge = np.zeros(plane.shape, dtype=bool)
            for da, db in ((-1, 0), (1, 0), (0, -1), (0, 1)):
                edge |= padded[1 + da:1 + da + plane.shape[0], 1 + db:1 + db + plane.shape[1]] != plane
            draw &= edge[a, b]
        A = rgba[..., 3:4]
        rgb = np.where(draw[..., None], (A * rgba[..., :3] + (255 - A) * rgb + 127) // 255, rgb)
    rgb = np.where(ok[..., None], rgb, 0).astype(np.uint8)
    r0, r1 = max(0, -t['y0']), min(t['h'], H - t['y0'])
    c0, c1 = max(0, -t['x0']), min(t['w'], W - t['x0'])
    if r1 > r0 and c1 > c0:
        canvas[t['y0'] + r0:t['y0'] + r1, t['x0'] + c0:t['x0'] + c1] = rgb[r0:r1, c0:c1]


def paint_tiles(tiles, H, W):
    """uint8 [H, W, 3]: a list of tile records painted over black.  A record is a dict: x0, y0, w, h (canvas
    rectangle), kind 'f32' (volume [X, Y, Z, C], channel, vmin, vmax) or 'u8' (volume [X, Y, Z], table), shape, axis,
    index, origin and step (row axis, column axis) and overlays [(volume, table, 'fill' | 'outline'), ...] (at most
    two).  Volumes that are HIP tensors (all of them, on one device): one ru3d_render_tiles launch."""
    if not tiles:
        return np.zeros((H, W, 3), dtype=np.uint8)
    device = _device_of(*[t['volume'] for t in tiles])
    if device is None:
        canvas = np.zeros((H, W, 3), dtype=np.uint8)
        for t in tiles:
            _paint_tile_numpy(canvas, t)
        return canvas
    import torch
    import _native as N
    from _native import check, ptr, stream
    if len(tiles) > N.RENDER_MAX_TILES:
        raise ValueError("paint_tiles: %d tiles (at most %d a launch)" % (len(tiles), N.RENDER_MAX_TILES))
    records = (N.RenderTile * len(tiles))()
    keep = {}

    def table_ptr(table):
        if id(table) not in keep:
            keep[id(table)] = torch.from_numpy(np.ascontiguousarray(table)).to(device)
        return keep[id(table)].data_ptr()

    def volume_ptr(v, dtype):
        if not _is_hip(v) or v.device != device or v.dtype != dtype or not v.is_contiguous():
            raise ValueError("paint_tiles: every volume of the device route must be a contiguous %s tensor on %s"
                             % (dtype, device))
        return v.data_ptr()

    for rec, t in zip(records, tiles):
        X, Y, Z = (int(s) for s in t['shape'])
        f32 = t['kind'] == 'f32'
        C = int(t['volume'].shape[3]) if f32 else 1
        if X * Y * Z * C >= 1 << 31:
            raise ValueError("paint_tiles: a volume of %d elements (fewer than 2**31)" % (X * Y * Z * C))
        if tuple(t['volume'].shape[:3]) != (X, Y, Z) or len(t['overlays']) > 2:
            raise ValueError("paint_tiles: bad tile record")
        rec.volume = volume_ptr(t['volume'], torch.float32 if f32 else torch.uint8)
        rec.table = None if f32 else table_ptr(t['table'])
        for o, (volume, table, mode) in enumerate(t['overlays']):
            if tuple(volume.shape) != (X, Y, Z):
                raise ValueError("paint_tiles: an overlay of shape %s over a volume of %s" % (tuple(volume.shape), (X, Y, Z)))
            rec.overlay[o] = volume_ptr(volume, torch.uint8)
            rec.overlay_table[o] = table_ptr(table)
            rec.overlay_mode[o] = N.OVERLAY_OUTLINE if mode == 'outline' else N.OVERLAY_FILL
        rec.vmin, rec.vmax = (float(t['vmin']), float(t['vmax'])) if f32 else (0.0, 1.0)
        rec.origin[0], rec.origin[1] = (float(v) for v in t['origin'])
        rec.step[0], rec.step[1] = (float(v) for v in t['step'])
        rec.x0, rec.y0, rec.w, rec.h = int(t['x0']), int(t['y0']), int(t['w']), int(t['h'])
        rec.X, rec.Y, rec.Z, rec.C = X, Y, Z, C
        rec.channel, rec.kind = (int(t['channel']), N.TILE_F32) if f32 else (0, N.TILE_U8)
        rec.axis, rec.index = int(t['axis']), int(t['index'])
    packed = torch.from_numpy(np.frombuffer(bytes(records), dtype=np.uint8).copy()).to(device)
    canvas = torch.zeros((H, W, 3), dtype=torch.uint8, device=device)
    N.note_device(device)
    check(N.lib.ru3d_render_tiles(ptr(packed), len(tiles), ptr(canvas), H, W, stream()), "render_tiles")
    return canvas.cpu().numpy()


def case_sheet(case, axes=(0, 1, 2), num_slices=8, window=None, overlays=('label', 'pred'), pixel_mm=None, colours=None):
    """uint8 [H, W, 3]: one row of `num_slices` equally spaced slices per axis of `axes` - spaced over the bounding box
    (in 8-voxel bricks) of the overlays when they hold anything, else over the volume -, channel 0 of the image in
    grey under the first overlay filled and the second outlined, in square pixels of `pixel_mm` millimetres (default:
    the longest side of the volume is 256 pixels) from the affine's spacing.  window=None: the 0.5 / 99.5 percentiles
    of the image.  Without an image the first overlay is the picture and the second is outlined over it."""
    present = [k for k in overlays if case.get(k) is not None]
    if len(present) > 2:
        raise ValueError("case_sheet: at most two overlays, got %r" % (present,))
    image = case.get('image')
    if image is None and not present:
        raise ValueError("case_sheet: the case holds neither an image nor one of %r" % (overlays,))
    device = _device_of(image, *[case[k] for k in present])
    if image is not None and len(image.shape) != 4:
        raise ValueError("case_sheet: case['image'] has shape %s ([X, Y, Z, C])" % (tuple(image.shape),))
    shape = tuple(int(s) for s in (image.shape[:3] if image is not None else case[present[0]].shape))
    if num_slices < 1 or not axes or any(a not in (0, 1, 2) for a in axes):
        raise ValueError("case_sheet: axes=%r, num_slices=%r" % (axes, num_slices))
    spacing = spacing_of(case)
    if device is None:
        image = _to_host(image, 'f32') if image is not None else None
        volumes = [_to_host(case[k], 'u8') for k in present]
    else:
        image = _to_device(image, device, 'f32') if image is not None else None
        volumes = [_to_device(case[k], device, 'u8') for k in present]
    for v in volumes:
        if tuple(v.shape) != shape:
            raise ValueError("case_sheet: an overlay of shape %s over a volume of %s" % (tuple(v.shape), shape))
    fill = colour_table(colours, 0.45)
    line = colour_table(colours, 1.0)
    every = colour_table(None, 1.0)
    bricks = None
    for v in volumes:
        b = _Prepared(v, every).bricks if device is not None else _bricks_numpy(v, every)
        bricks = b if bricks is None else bricks | b
    box = _brick_box(bricks, shape) if bricks is not None else None
    lo, hi = box if box is not None else ([0, 0, 0], list(shape))
    base = {'shape': shape}
    if image is not None:
        if window is None:
            window = [float(p) for p in _percentiles(image, (0.5, 99.5))]
        base.update(kind='f32', volume=image, channel=0, vmin=float(window[0]), vmax=float(window[1]),
                    overlays=[(v, t, m) for v, t, m in zip(volumes, (fill, line), ('fill', 'outline'))])
    else:
        base.update(kind='u8', volume=volumes[0], table=line,
                    overlays=[(v, line, 'outline') for v in volumes[1:]])
    if pixel_mm is None:
        pixel_mm = max(shape[c] * spacing[c] for c in range(3)) / 256.0
    pixel_mm = float(pixel_mm)
    if not pixel_mm > 0:
        raise ValueError("case_sheet: pixel_mm=%r" % (pixel_mm,))
    tiles, gap, y = [], 2, 0
    width = 0
    for axis in axes:
        ax_a, ax_b = _in_plane(axis)
        h = max(1, int(math.ceil(shape[ax_a] * spacing[ax_a] / pixel_mm)))
        w = max(1, int(math.ceil(shape[ax_b] * spacing[ax_b] / pixel_mm)))
        step = (pixel_mm / spacing[ax_a], pixel_mm / spacing[ax_b])
        count = hi[axis] - lo[axis]
        for k in range(num_slices):
            tiles.append(dict(base, axis=axis, index=lo[axis] + ((2 * k + 1) * count) // (2 * num_slices),
                              x0=k * (w + gap), y0=y, w=w, h=h, origin=(0.5 * step[0], 0.5 * step[1]), step=step))
        width = max(width, num_slices * (w + gap) - gap)
        y += h + gap
    return paint_tiles(tiles, y - gap, width)


# ----------------------------------------------------------------------------------------------- shaded views
def view_vectors(azimuth, elevation):
    """(u, v, w): unit vectors of the picture's columns (rightwards), rows (downwards) and of the viewing direction, in
    the volume's millimetre frame, for a camera at `azimuth` degrees about the z axis and `elevation` degrees above the
    x-y plane.  The only transcendental functions of the renderer: evaluated here, on the host, for both routes."""
    az, el = math.radians(azimuth), math.radians(elevation)
    c = np.array([math.cos(el) * math.cos(az), math.cos(el) * math.sin(az), math.sin(el)])
    u = np.array([-math.sin(az), math.cos(az), 0.0])
    return u, -np.cross(c, u), -c


def fit_view(box, spacing, azimuth, elevation, size, ambient=0.25, diffuse=0.75, background=(0, 0, 0)):
    """The ru3d_render_view terms, as a dict of float64 vectors in voxel units, of a size x size picture whose view box
    holds the voxel box `box` = (lo, hi): pixels 4 % larger than the tight fit, samples half the smallest spacing
    apart, starting one sample in front of the box; the light comes from above the viewer's left shoulder."""
    spacing = np.asarray(spacing, dtype=np.float64)
    lo, hi = (np.asarray(b, dtype=np.float64) for b in box)
    u, v, w = view_vectors(azimuth, elevation)
    centre, half = (lo + hi) / 2.0 * spacing, (hi - lo) / 2.0 * spacing
    hu, hv, hw = (float(np.abs(d) @ half) for d in (u, v, w))
    pixel = 2.0 * max(hu, hv) * 1.04 / size
    step = 0.5 * float(spacing.min())
    origin = centre - ((size - 1) / 2.0 * pixel) * (u + v) - (hw + step) * w
    light = -w - 0.4 * u - 0.5 * v
    return {'o': origin / spacing, 'du': pixel * u / spacing, 'dv': pixel * v / spacing, 'dw': step * w / spacing,
            'spacing': spacing, 'light': light / math.sqrt(float(light @ light)), 'ambient': float(ambient),
            'diffuse': float(diffuse), 'background': np.asarray(background, dtype=np.float64),
            'num_steps': int(math.ceil(2.0 * (hw + step) / step)) + 1}


def cast_numpy(volume, table, view, H, W, u0=0, v0=0):
    """(rgb uint8 [H, W, 3], depth int32 [H, W]) of a uint8 volume: the contract of ru3d_render_surface in numpy, one
    vectorised pass over the picture per sample number.  The definition, not a product.  (u0, v0): the picture's
    first column and row, for rendering a rectangle of a larger picture."""
    X, Y, Z = volume.shape
    ext = (X, Y, Z)
    drawn = table[:, 3] != 0
    drawn[0] = False
    padded = np.pad(volume, 1)
    cols = np.arange(u0, u0 + W, dtype=np.float64)[None, :]
    rows = np.arange(v0, v0 + H, dtype=np.float64)[:, None]
    base = [(view['o'][c] + cols * view['du'][c]) + rows * view['dv'][c] for c in range(3)]
    T = np.ones((H, W))
    C = np.zeros((H, W, 3))
    depth = np.full((H, W), -1, dtype=np.int32)
    prev = np.zeros((H, W), dtype=np.int64)
    alive = np.ones((H, W), dtype=bool)
    light, spacing = view['light'], view['spacing']
    for n in range(int(view['num_steps'])):
        f = [np.floor(base[c] + np.float64(n) * view['dw'][c]) for c in range(3)]
        inside = np.ones((H, W), dtype=bool)
        for c in range(3):
            inside &= (f[c] >= 0) & (f[c] < ext[c])
        p = [np.where(inside, f[c], 0).astype(np.int64) for c in range(3)]
        L = np.where(inside, volume[p[0], p[1], p[2]], 0).astype(np.int64)
        event = alive & drawn[L] & (L != prev)
        prev = L
        if not event.any():
            continue
        e = [q[event] for q in p]
        Le = L[event]
        g = np.zeros((3, len(Le)), dtype=np.int64)
        for dx in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dz in (-1, 0, 1):
                    occ = padded[e[0] + 1 + dx, e[1] + 1 + dy, e[2] + 1 + dz] == Le
                    g[0] += dx * occ
                    g[1] += dy * occ
                    g[2] += dz * occ
        m = [(-g[c]).astype(np.float64) / spacing[c] for c in range(3)]
        dot = (m[0] * light[0] + m[1] * light[1]) + m[2] * light[2]
        len2 = (m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]
        with np.errstate(all='ignore'):
            lit = view['ambient'] + (view['diffuse'] * np.maximum(dot, 0.0)) / np.sqrt(len2)
        shade = np.where(len2 == 0, view['ambient'] + view['diffuse'], lit)
        a = table[Le, 3].astype(np.float64) / 255.0
        k = (T[event] * a) * shade
        for c in range(3):
            C[..., c][event] = C[..., c][event] + k * table[Le, c].astype(np.float64)
        T[event] = T[event] * (1.0 - a)
        depth[event & (depth < 0)] = n
        alive &= T >= 1.0 / 256.0
        if not alive.any():
            break
    out = C + T[..., None] * np.asarray(view['background'], dtype=np.float64)
    return np.floor(np.minimum(np.maximum(out, 0.0), 255.0) + 0.5).astype(np.uint8), depth


def cast_device(prepared, view, H, W):
    """(rgb, depth) as numpy arrays: one ru3d_render_surface launch on a `_Prepared` volume."""
    import torch
    import _native as N
    from _native import check, ptr, stream
    volume = prepared.volume
    X, Y, Z = volume.shape
    vw = N.RenderView()
    for name in ('o', 'du', 'dv', 'dw', 'spacing', 'light', 'background'):
        for c in range(3):
            getattr(vw, name)[c] = float(view[name][c])
    vw.ambient, vw.diffuse, vw.num_steps = float(view['ambient']), float(view['diffuse']), int(view['num_steps'])
    rgb = torch.empty((H, W, 3), dtype=torch.uint8, device=volume.device)
    depth = torch.empty((H, W), dtype=torch.int32, device=volume.device)
    N.note_device(volume.device)
    check(N.lib.ru3d_render_surface(ptr(volume), X, Y, Z, ptr(prepared.table), ctypes.byref(vw), ptr(rgb), ptr(depth), H, W,
                                    ptr(prepared.ws), prepared.ws.numel(), stream()), "render_surface")
    return rgb.cpu().numpy(), depth.cpu().numpy()


def render_case(case, key='pred', labels=None, views=((30, 20),), size=512, alpha=None, colours=None, return_depth=False):
    """uint8 [len(views), size, size, 3]: shaded orthographic views (azimuth, elevation in degrees) of the label volume
    case[key], the view box fitted to the bounding box (in 8-voxel bricks) of the drawn labels.  labels=None draws every
    non-zero label; alpha: None (opaque: the first surface hit), one number, or {label: number} - 0.35 on the kidney
    shows what lies inside it.  An empty selection gives the background.  return_depth=True: (pictures, int32
    [len(views), size, size] sample number of the first surface, -1 where there is none)."""
    volume = case[key]
    if len(volume.shape) != 3:
        raise ValueError("render_case: case[%r] has shape %s ([X, Y, Z])" % (key, tuple(volume.shape)))
    size = int(size)
    if size < 1:
        raise ValueError("render_case: size=%r" % (size,))
    table = colour_table(colours, alpha, labels)
    spacing = spacing_of(case)
    if _is_hip(volume):
        prepared = _Prepared(_to_device(volume, volume.device, 'u8'), table)
        bricks = prepared.bricks
    else:
        volume = _to_host(volume, 'u8')
        bricks = _bricks_numpy(volume, table)
    box = _brick_box(bricks, volume.shape)
    pictures = np.zeros((len(views), size, size, 3), dtype=np.uint8)
    depths = np.full((len(views), size, size), -1, dtype=np.int32)
    for i, (azimuth, elevation) in enumerate(views):
        if box is None:
            continue
        view = fit_view(box, spacing, azimuth, elevation, size)
        pictures[i], depths[i] = cast_device(prepared, view, size, size) if _is_hip(volume) else \
            cast_numpy(volume, table, view, size, size)
    return (pictures, depths) if return_depth else pictures
