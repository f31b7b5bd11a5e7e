"""Volumes shared by test_host_postprocess.py and test_gpu_postprocess.py: masks with known holes, label maps with
cavities, enclosed classes and specks, and three tiny validation cases written with the project's NIfTI writer."""
import os

import numpy as np
import scipy.ndimage as ndi

CROSS = None
CUBE = np.ones((3, 3, 3), dtype=bool)


def smooth_noise():
    return ndi.gaussian_filter(np.random.RandomState(0).standard_normal((37, 45, 150)), 1.0) > -0.05


def dense_noise():
    return np.random.RandomState(5).rand(21, 33, 131) < 0.7


def hollow_box(clear=None):
    h = np.zeros((12, 12, 70), dtype=bool)
    h[2:10, 2:10, 30:40] = 1
    h[3:9, 3:9, 31:39] = 0
    if clear is not None:
        h[clear] = 0
    return h


def serpentine(opened):
    """A solid block with a one-voxel channel winding through the plane z = 35: y = 1 .. 38 on every odd x up to 37,
    each column joined to the next at x + 1, alternately at y = 38 and y = 1 (the last join is a dead end at x = 38)."""
    s = np.ones((40, 40, 70), dtype=bool)
    for i, x in enumerate(range(1, 38, 2)):
        s[x, 1:39, 35] = 0
        s[x + 1, 38 if i % 2 == 0 else 1, 35] = 0
    if opened:
        s[0, 1, 35] = 0
    return s


def ring2d():
    r = np.zeros((20, 140), dtype=bool)
    r[5:15, 60:70] = 1
    r[6:14, 61:69] = 0
    return r


def toy_kidney():
    """A box kidney (1) whose cavity of 57 voxels holds a tumour (2, 45 voxels) and 12 background voxels."""
    v = np.zeros((14, 14, 16), dtype=np.uint8)
    v[2:12, 2:12, 2:14] = 1
    v[5:8, 5:8, 4:9] = 2
    v[5:8, 5:9, 9:10] = 0
    return v


def three_class_map():
    """(32, 40, 130), classes 1 .. 3: two kidneys with background cavities, a tumour enclosed in the first, an aorta
    with a closed lumen that joins them into one foreground component, and far specks of every class."""
    v = np.zeros((32, 40, 130), dtype=np.uint8)
    x, y, z = np.ogrid[:32, :40, :130]
    v[((x - 15) / 11.0) ** 2 + ((y - 12) / 9.0) ** 2 + ((z - 35) / 25.0) ** 2 <= 1] = 1
    v[((x - 16) / 10.0) ** 2 + ((y - 28) / 8.0) ** 2 + ((z - 95) / 24.0) ** 2 <= 1] = 1
    v[12:17, 9:14, 28:36] = 2                                   # enclosed in the first kidney
    v[14:18, 11:15, 44:50] = 0                                  # cavities
    v[13:15, 26:30, 60:68] = 0                                  # spans the word boundary at z = 64
    v[16:19, 27:29, 100:104] = 0
    v[10:14, 18:22, :] = 3                                      # the aorta runs through the volume: open at both faces
    v[11:13, 19:21, 70:90] = 0                                  # its lumen reaches no face: a hole of class 3
    v[2:4, 2:4, 2:4] = 1                                        # specks
    v[28:30, 35:38, 120:123] = 1
    v[29, 2, 64] = 2
    v[1:3, 36:38, 60:62] = 3
    v[25:27, 3:5, 100:103] = 2
    return v


def validation_cases():
    """Three (label, pred) pairs of classes 0 .. 2 on (12, 14, 40).
      0: two kidneys; the prediction adds a speck of class 1 glued to the far side of the tumour, so the foreground has
         two components and class 1 three: keeping one component of class 1 loses a kidney, keeping two drops the speck.
      1: one kidney, no tumour anywhere; the prediction adds a far speck: foreground clean-up removes it.
      2: the prediction misses a slab of the kidney and has nothing spurious: no step gains anything."""
    cases = []
    label = np.zeros((12, 14, 40), dtype=np.uint8)
    label[2:8, 2:8, 3:12] = 1
    label[3:6, 3:6, 12:15] = 2
    label[2:8, 2:8, 25:34] = 1
    pred = label.copy()
    pred[4, 4, 15:17] = 1
    cases.append((label, pred))
    label = np.zeros((12, 14, 40), dtype=np.uint8)
    label[3:9, 4:10, 10:20] = 1
    pred = label.copy()
    pred[10:12, 12:14, 36:39] = 1
    cases.append((label, pred))
    label = np.zeros((12, 14, 40), dtype=np.uint8)
    label[3:9, 4:10, 10:20] = 1
    label[5:7, 6:8, 20:23] = 2
    pred = label.copy()
    pred[3:9, 4:10, 10:12] = 0
    cases.append((label, pred))
    return cases


def write_validation_cases(root):
    """-> (label_dir, pred_dir) holding case_0 .. case_2 as NIfTI files."""
    import nifti
    label_dir, pred_dir = os.path.join(str(root), "labels"), os.path.join(str(root), "preds")
    os.makedirs(label_dir)
    os.makedirs(pred_dir)
    for i, (label, pred) in enumerate(validation_cases()):
        nifti.save(label, np.eye(4), os.path.join(label_dir, "case_%d.label.nii.gz" % i))
        nifti.save(pred, np.eye(4), os.path.join(pred_dir, "case_%d.pred.nii.gz" % i))
    return label_dir, pred_dir


def holes(mask, structure):
    return int(ndi.binary_fill_holes(mask, structure=structure).sum() - mask.sum())


def keep_largest_numpy(mask, k):
    """The numpy twin of components.keep_largest: (kept mask, relabelled survivors)."""
    labels, _ = ndi.label(mask)
    sizes = np.bincount(labels.ravel())[1:]
    chosen = np.sort(np.argsort(-sizes, kind='stable')[:k]) + 1
    kept = np.isin(labels, chosen)
    return kept, ndi.label(kept)[0]
