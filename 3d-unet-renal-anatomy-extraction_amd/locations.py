"""Foreground oversampling of the patch sampler, host side: the class-location index of a case in plain numpy, the
argument checks, and the draws that turn an index into a crop box.  `augment.DeviceAugment` (index: ru3d_class_index,
csrc/locations.hip) and the numpy crops of `transform` share this module, so one seed gives one patch on both.

The index of a label volume [X, Y, Z], linear index i = (x * Y + y) * Z + z, for the values c = 0 .. 31:
    counts[c]     the number of voxels with value c (other values are counted nowhere and appear nowhere);
    boxes[c]      (x0, x1, y0, y1, z0, z1), low end inclusive, high end exclusive; zeros for an absent class;
    locations[c]  m = min(counts[c], max_per_class) linear indices: np.flatnonzero(label == c)[(np.arange(m) * n) // m],
                  the complete raster-ordered list of a class of at most max_per_class voxels, an evenly rank-strided
                  subsample of a larger one.  No random numbers: the kernel and this module agree voxel for voxel.

The draws of a patch with oversample_foreground = p, after the scale (and with it `before`, the box size):
    u = rng.uniform(); the patch is forced iff u < p;
    forced, and the case has eligible classes E (ascending; foreground_classes, or every value >= 1, present in the
    case): c = E[rng.randint(0, len(E))], j = rng.randint(0, len(locations[c])), v = unravel(locations[c][j]), and per axis,
    with hi = shape - before - margin: lo = min(max(v - before // 2, margin), hi) if hi > margin else
    (shape - before) // 2.  No further draw for the box.  The upper clamp is hi itself (not hi - 1, the largest corner
    a random box gets from randint's exclusive bound): with margin 0 the voxel always lies in [lo, lo + before);
    otherwise the box is drawn as without oversampling.
"""
import numpy as np

NUM_CLASSES = 32                # RU3D_CLASS_INDEX_CLASSES
MAX_PER_CLASS = 1 << 20         # RU3D_CLASS_INDEX_MAX_PER_CLASS


def check_max_locations(max_per_class):
    m = int(max_per_class)
    if m != max_per_class or not 1 <= m <= MAX_PER_CLASS:
        raise ValueError("max_locations %r (an integer in 1 .. %d)" % (max_per_class, MAX_PER_CLASS))
    return m


def class_locations(label, max_per_class=10000):
    """(counts int64 [32], boxes int32 [32, 6], [locations of class c: int32 [m_c] for c in 0 .. 31]) of an integer
    label volume [X, Y, Z]: the contract of ru3d_class_index in numpy."""
    m_max = check_max_locations(max_per_class)
    label = np.asarray(label)
    if label.ndim != 3:
        raise ValueError("class_locations: a label volume [X, Y, Z], not %s" % (label.shape,))
    flat = label.reshape(-1)
    counts = np.zeros(NUM_CLASSES, dtype=np.int64)
    boxes = np.zeros((NUM_CLASSES, 6), dtype=np.int32)
    rows = []
    present = np.unique(flat)
    for c in range(NUM_CLASSES):
        if c not in present:
            rows.append(np.zeros(0, dtype=np.int32))
            continue
        where = np.flatnonzero(flat == c)
        n = where.size
        m = min(n, m_max)
        counts[c] = n
        rows.append(where[(np.arange(m, dtype=np.int64) * n) // m].astype(np.int32))
        xyz = np.unravel_index(where, label.shape)
        boxes[c] = [v for a in xyz for v in (a.min(), a.max() + 1)]
    return counts, boxes, rows


def check_oversample(oversample_foreground, foreground_classes, max_locations, crop_mode, enforce_label_indices):
    """-> (p | None, sorted class list | None, max_locations); ValueError for what the rule does not cover."""
    m = check_max_locations(max_locations)
    if oversample_foreground is None:
        return None, None, m
    p = float(oversample_foreground)
    if not 0 < p <= 1:
        raise ValueError("oversample_foreground %r (None or a probability in (0, 1])" % (oversample_foreground,))
    if len(enforce_label_indices) > 0:
        raise ValueError("oversample_foreground replaces enforce_label_indices: give one of the two")
    if crop_mode != "random":
        raise ValueError("oversample_foreground needs crop_mode='random' (a centre crop has no box to place)")
    classes = None
    if foreground_classes is not None:
        if any(int(c) != c or not 1 <= c < NUM_CLASSES for c in foreground_classes):
            raise ValueError("foreground_classes %r (label values in 1 .. %d)" % (foreground_classes, NUM_CLASSES - 1))
        classes = sorted(set(int(c) for c in foreground_classes))
    return p, classes, m


def eligible(counts, classes):
    """The classes a forced patch may pick in a case with these counts, ascending."""
    if classes is None:
        return [c for c in range(1, NUM_CLASSES) if counts[c] > 0]
    return [c for c in classes if counts[c] > 0]


def forced_box(voxel, before, shape, margin):
    """The lower corner of the crop box of size `before` placed on `voxel` (three indices) in a volume of `shape`."""
    lo = []
    for i in range(3):
        hi = shape[i] - before[i] - margin[i]
        if hi > margin[i]:
            lo.append(int(min(max(voxel[i] - before[i] // 2, margin[i]), hi)))
        else:
            lo.append(int((shape[i] - before[i]) // 2))
    return lo


def draw_forced_box(rng, p, classes, index, before, shape, margin):
    """The oversampling draws of one patch.  index: a callable -> (counts, locations(c)) of the case, called only on a
    forced patch.  Returns the box's lower corner, or None when the box is to be drawn the usual way."""
    if not rng.uniform() < p:
        return None
    counts, locations = index()
    choice = eligible(counts, classes)
    if not choice:
        return None
    c = choice[int(rng.randint(0, len(choice)))]
    row = locations(c)
    v = int(row[int(rng.randint(0, len(row)))])
    voxel = (v // (shape[1] * shape[2]), (v // shape[2]) % shape[1], v % shape[2])
    return forced_box(voxel, before, shape, margin)
