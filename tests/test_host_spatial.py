"""CPU-only checks of the free-form spatial transform (rotation, per-axis zoom, cubic B-spline elastic deformation):
the numpy route (`spatial`, re-exported by `transform`) against scipy.ndimage.map_coordinates and against
RandomRescaleCrop, the argument checks of DeviceAugment / RandomSpatialCrop and of the C entry point (no launch), and the
header / binding / export of `ru3d_augment_patch_spatial`."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import scipy.ndimage as ndi

import _native as N
import augment
import spatial
import transform

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ geometry
def test_rotation_matrix_is_a_right_handed_rotation():
    rng = np.random.RandomState(0)
    for ax, ay, az in rng.uniform(-np.pi, np.pi, size=(8, 3)):
        r = transform.rotation_matrix(ax, ay, az)
        assert r.dtype == np.float64 and np.abs(r @ r.T - np.eye(3)).max() <= 1e-14
        assert abs(np.linalg.det(r) - 1.0) <= 1e-14
        want = transform.rotation_matrix(0, 0, az) @ transform.rotation_matrix(0, ay, 0) @ transform.rotation_matrix(ax, 0, 0)
        assert np.abs(r - want).max() <= 1e-15                                  # Rz . Ry . Rx
        other = transform.rotation_matrix(ax, 0, 0) @ transform.rotation_matrix(0, ay, 0) @ transform.rotation_matrix(0, 0, az)
        assert np.abs(r - other).max() > 1e-3
    q = np.pi / 2
    x, y, z = np.eye(3)
    assert np.allclose(transform.rotation_matrix(q, 0, 0) @ y, z, atol=1e-15)   # Rx: y -> z
    assert np.allclose(transform.rotation_matrix(q, 0, 0) @ x, x, atol=1e-15)
    assert np.allclose(transform.rotation_matrix(0, q, 0) @ z, x, atol=1e-15)   # Ry: z -> x
    assert np.allclose(transform.rotation_matrix(0, 0, q) @ x, y, atol=1e-15)   # Rz: x -> y
    assert np.array_equal(transform.rotation_matrix(0, 0, 0), np.eye(3))


@pytest.mark.parametrize("patch,g", [((37, 50, 65), (4, 16, 32)), ((17, 1, 33), (4, 4, 16)), ((5, 64, 80), (16, 32, 4))])
def test_bspline_displacement_is_the_uniform_cubic_bspline(patch, g):
    rng = np.random.RandomState(1)
    n = spatial.lattice_shape(patch, g)
    phi = rng.randn(3, *n).astype(np.float32)
    d = transform.bspline_displacement(phi, g, patch)
    assert d.shape == (3,) + patch and d.dtype == np.float64
    t = np.stack(np.meshgrid(*[np.arange(p) / s for p, s in zip(patch, g)], indexing="ij"))
    for k in range(3):
        want = ndi.map_coordinates(phi[k].astype(np.float64), t + 1, order=3, prefilter=False, mode="nearest")
        assert np.abs(d[k] - want).max() <= 1e-12
    shift = np.broadcast_to(np.array([1.5, -2.0, 0.25], dtype=np.float32).reshape(3, 1, 1, 1), (3,) + n)
    d = transform.bspline_displacement(shift, g, patch)
    assert np.abs(d - shift[:, :1, :1, :1]).max() <= 1e-14                      # partition of unity: a pure shift
    assert not transform.bspline_displacement(np.zeros((3,) + n, np.float32), g, patch).any()
    with pytest.raises(ValueError, match="phi"):
        transform.bspline_displacement(phi[:, :-1], g, patch)


def test_lattice_extents():
    want = {(1, 4): 3, (5, 4): 4, (64, 4): 19, (80, 4): 23, (128, 4): 35, (160, 4): 43,
            (1, 16): 3, (5, 16): 4, (64, 16): 7, (80, 16): 8, (128, 16): 11, (160, 16): 13,
            (1, 32): 3, (5, 32): 4, (64, 32): 5, (80, 32): 6, (128, 32): 7, (160, 32): 8}
    for (p, g), n in want.items():
        assert spatial.lattice_shape((p, p, p), (g, g, g)) == (n, n, n), (p, g)
        # every voxel's four taps lie inside, or (last voxel of a whole number of cells) the fourth has weight 0
        assert (p - 1) // g + 3 <= n - 1 or (p - 1) % g == 0


@pytest.mark.parametrize("flip", [None, (1, 0, 1), (0, 1, 0), (1, 1, 1)])
def test_identity_coordinates_are_the_rescale_crop_grid(flip):
    patch, lo, before = (37, 50, 65), np.array([3, -4, 11]), np.array([41, 46, 70])
    centre, matrix = spatial.patch_geometry(lo, before, patch)
    s = transform.spatial_coordinates(patch, centre, matrix, flip=flip)
    axes = []
    for d in range(3):
        o = np.arange(patch[d], dtype=np.float64)
        if flip is not None and flip[d]:
            o = patch[d] - 1 - o
        axes.append(lo[d] + o * ((before[d] - 1) / (patch[d] - 1)))
    want = np.stack(np.meshgrid(*axes, indexing="ij"))
    assert s.shape == (3,) + patch and s.dtype == np.float64
    assert np.abs(s - want).max() <= 1e-12 * 128
    c1, m1 = spatial.patch_geometry([0, 0, 0], [9, 9, 9], (1, 4, 4))            # P == 1: step 0, the box's centre
    assert m1[0, 0] == 0 and transform.spatial_coordinates((1, 4, 4), c1, m1)[0].max() == 4.0


def test_mirrored_coordinates_carry_the_lattice():
    """out[o] reads what the unmirrored patch reads at o' = P - 1 - o, displacement included."""
    rng = np.random.RandomState(2)
    patch, g = (12, 9, 20), (4, 4, 8)
    phi = rng.randn(3, *spatial.lattice_shape(patch, g)).astype(np.float32)
    centre, matrix = spatial.patch_geometry([1, 2, 3], [14, 8, 25], patch, (0.1, -0.2, 0.3))
    plain = transform.spatial_coordinates(patch, centre, matrix, phi, g)
    flipped = transform.spatial_coordinates(patch, centre, matrix, phi, g, flip=(1, 0, 1))
    assert np.array_equal(flipped, plain[:, ::-1, :, ::-1])


# ------------------------------------------------------------------------------------------------ resampling
def test_resample_at_images_against_map_coordinates():
    rng = np.random.RandomState(3)
    vol = rng.randn(30, 28, 26).astype(np.float32)
    coords = rng.uniform(-6, 36, size=(3, 24, 20, 22))
    coords[:, 0, 0, :4] = [[-1000.0] * 4, [5.0] * 4, [1e9, -1e9, 40.0, 13.5]]   # far outside the volume
    coords[:, 1] = np.round(coords[:, 1])                                        # on the grid
    got = transform.resample_at(vol, coords, cval=1.5)
    want = ndi.map_coordinates(vol.astype(np.float64), coords, order=1, mode="grid-constant", cval=1.5)
    assert got.dtype == np.float32 and got.shape == (24, 20, 22)
    assert np.abs(got - want).max() <= 1e-6
    assert (got[0, 0, :4] == 1.5).all()
    two = np.stack([vol, -2 * vol], axis=-1)
    got2 = transform.resample_at(two, coords, cval=1.5, chunk=1000)              # chunking changes nothing
    assert got2.shape == (24, 20, 22, 2) and np.array_equal(got2[..., 0], got)


@pytest.mark.parametrize("tag", ["iia_like", "binary_label", "pads", "center_two_ch", "margin_enforce"])
def test_identity_spatial_crop_is_random_rescale_crop_on_g7(golden_dir, tag):
    """Zero-width rotation ranges and magnitude (0, 0): the same scale and box draws, then the identity geometry -
    RandomRescaleCrop's patch (image 2e-6, labels identical, the label rule of transform.rescale included)."""
    z = np.load(os.path.join(golden_dir, "g7_augment.npz"))
    kw = {"iia_like": dict(scale=0.1, crop_mode="random"), "binary_label": dict(scale=0.2, crop_mode="random"),
          "pads": dict(scale=0.1, crop_mode="random"), "center_two_ch": dict(scale=[0.8, 1.3], crop_mode="center"),
          "margin_enforce": dict(scale=0.1, crop_mode="random", crop_margin=4, enforce_label_indices=[2])}[tag]
    patch = [int(v) for v in z[tag + "/patch"]]
    image, label, seed = z[tag + "/image_in"], z[tag + "/label_in"], int(z[tag + "/seed"])
    np.random.seed(seed)
    want = transform.RandomRescaleCrop(crop_size=list(patch), **kw)({"image": image.copy(), "label": label.copy()})
    np.random.seed(seed)
    got = transform.RandomSpatialCrop(crop_size=list(patch), rotation=((0, 0), (0, 0), (0, 0)), elastic_spacing=8,
                                      elastic_magnitude=(0, 0), **kw)({"image": image.copy(), "label": label.copy()})
    assert got["image"].shape == want["image"].shape and got["image"].dtype == want["image"].dtype
    assert np.abs(got["image"] - want["image"]).max() <= 2e-6
    assert got["label"].dtype == want["label"].dtype and np.array_equal(got["label"], want["label"])


def test_label_rule_ties_and_margin():
    lab = np.zeros((4, 4, 4), np.uint8)
    lab[2:] = 3
    lab[:, 2:] += 1                                                               # classes 0, 1, 3, 4
    coords = np.array([[1.5, 1.5, 1.0], [1.25, 1.25, 1.0], [1.25, 1.5, 1.0], [9.0, 9.0, 9.0]]).T.reshape(3, 4, 1, 1)
    got, margin = transform.resample_at(lab, coords, cval=2, is_label=True, return_margin=True)
    assert got.ravel().tolist() == [0, 0, 0, 2]                                  # ties: the smallest class
    assert margin.ravel().tolist() == [0.0, 0.375, 0.0, 1.0]
    binary = (lab > 0).astype(np.int64)
    got = transform.resample_at(binary, coords, is_label=True)                   # two classes: interpolate and truncate
    assert got.dtype == np.int64 and got.ravel().tolist() == [0, 0, 0, 0]
    assert transform.resample_at(binary, np.full((3, 1, 1, 1), 3.0), is_label=True).item() == 1


def test_spatial_crop_draw_order():
    """scale, box, three angles, magnitude, lattice - then whatever follows (mirror, intensity) sees the same stream."""
    rng = np.random.RandomState(5)
    image = rng.randn(40, 36, 32, 1).astype(np.float32)
    label = (rng.rand(40, 36, 32) * 3).astype(np.uint8)
    np.random.seed(9)
    transform.RandomSpatialCrop(0.1, [16, 20, 12], rotation=0.2, elastic_spacing=4, elastic_magnitude=(1, 2),
                                crop_mode="random")({"image": image, "label": label})
    after = np.random.uniform()
    np.random.seed(9)
    np.random.uniform(0.9, 1.1)
    for _ in range(3):
        np.random.randint(0, 5)
    angles = [np.random.uniform(-0.2, 0.2) for _ in range(3)]
    m = np.random.uniform(1, 2)
    phi = (np.random.uniform(-1, 1, size=(3,) + spatial.lattice_shape([16, 20, 12], [4, 4, 4])) * m).astype(np.float32)
    assert np.random.uniform() == after
    assert phi.dtype == np.float32 and np.abs(phi).max() <= 2 and max(abs(a) for a in angles) <= 0.2
    # rotation=None with a lattice still draws three angles, from (0, 0)
    state = np.random.RandomState(3)
    got, phi2 = spatial.draw_spatial(state, None, ([8, 8, 8], (0.0, 1.0)), [16, 16, 16])
    assert got == [0.0, 0.0, 0.0] and phi2.shape == (3, 5, 5, 5)
    state2 = np.random.RandomState(3)
    state2.uniform(size=3)
    assert state2.uniform(0.0, 1.0) * 0 == 0 and np.array_equal(
        phi2, (np.random.RandomState(3).uniform(size=4)[3] * (state2.uniform(-1, 1, size=(3, 5, 5, 5)))).astype(np.float32))


# ------------------------------------------------------------------------------------------------ refusals
def test_python_refusals_name_the_argument():
    for bad in (-0.1, float("nan"), "x", ((0, 1), (0, 1)), ((1, 0), (0, 0), (0, 0)), ((0, float("inf")), (0, 0), (0, 0))):
        with pytest.raises(ValueError, match="rotation"):
            augment.DeviceAugment(rotation=bad)
        with pytest.raises(ValueError, match="rotation"):
            transform.RandomSpatialCrop(0.1, rotation=bad)
    for spacing, magnitude, word in ((16, None, "go together"), (None, (0, 1), "go together"), (3, (0, 1), "elastic_spacing"),
                                     ((16, 16), (0, 1), "elastic_spacing"), (16.0, (0, 1), "elastic_spacing"),
                                     ((16, 2, 16), (0, 1), "elastic_spacing"), (16, (2, 1), "elastic_magnitude"),
                                     (16, (-1, 1), "elastic_magnitude"), (16, 4, "elastic_magnitude"),
                                     (16, (0, float("nan")), "elastic_magnitude")):
        with pytest.raises(ValueError, match=word):
            augment.DeviceAugment(elastic_spacing=spacing, elastic_magnitude=magnitude)
        with pytest.raises(ValueError, match=word):
            transform.RandomSpatialCrop(0.1, elastic_spacing=spacing, elastic_magnitude=magnitude)
    # the kernel's lattice bound, known when the patch is: (ny + 4) * nz <= 2560
    augment.DeviceAugment(crop_size=128, elastic_spacing=4, elastic_magnitude=(0, 1))
    augment.DeviceAugment(crop_size=256, elastic_spacing=16, elastic_magnitude=(0, 1))
    augment.DeviceAugment(crop_size=[5, 133, 245], elastic_spacing=4, elastic_magnitude=(0, 1))
    for crop in (192, [5, 133, 249], [5, 137, 245]):
        with pytest.raises(ValueError, match="elastic_spacing.*2560"):
            augment.DeviceAugment(crop_size=crop, elastic_spacing=4, elastic_magnitude=(0, 1))
    assert spatial.MAX_YZ == N.SPATIAL_MAX_YZ == 2560


def test_new_keywords_default_to_none():
    sig = inspect.signature(augment.DeviceAugment.__init__)
    for name in ("rotation", "elastic_spacing", "elastic_magnitude"):
        assert sig.parameters[name].default is None, name
    assert list(sig.parameters)[:13] == ["self", "scale", "crop_size", "crop_mode", "crop_margin", "enforce_label_indices",
                                         "image_pad_cval", "label_pad_cval", "mirror_p", "contrast", "brightness", "gamma",
                                         "rng"]
    plain = augment.DeviceAugment()
    assert plain.rotation is None and plain.elastic is None and not plain.spatial
    assert transform.DeviceAugment is augment.DeviceAugment and transform.RandomSpatialCrop.__mro__[1] is transform.Crop
    assert list(inspect.signature(augment.DeviceAugment.sample).parameters) == ["self", "case", "out_image", "out_label"]


# ------------------------------------------------------------------------------------------------ entry point
def test_header_library_and_binding_name_the_entry_point():
    text = open(os.path.join(ROOT, "include", "ru3d.h")).read()
    assert re.search(r"\bru3d_augment_patch_spatial\s*\(", text) and "typedef struct ru3d_spatial_params" in text
    assert "#define RU3D_SPATIAL_MAX_YZ 2560" in text
    assert "ru3d_augment_patch_spatial" in N.SIGNATURES and len(N.SIGNATURES["ru3d_augment_patch_spatial"][1]) == 16
    assert hasattr(ctypes.CDLL(N.LIB_PATH), "ru3d_augment_patch_spatial")
    assert ctypes.sizeof(N.SpatialParams) == 12 * 8 + 6 * 4
    assert "augment.hip" in open(os.path.join(ROOT, "tools", "isa_check.py")).read()
    assert N.lib.ru3d_version() == 201


def test_c_argument_checks_answer_before_any_launch():
    lib = N.lib
    fake, other = ctypes.c_void_p(4096), ctypes.c_void_p(8192)                  # never dereferenced on these paths
    big = 1 << 30

    def params(patch=(16, 16, 16), lattice=(0, 0, 0), spacing=(0, 0, 0)):
        pr, sp = N.PatchParams(), N.SpatialParams()
        pr.patch[:] = patch
        sp.matrix[:] = np.eye(3).reshape(-1).tolist()
        sp.lattice[:], sp.spacing[:] = lattice, spacing
        return pr, sp

    def call(pr, sp, image=fake, label=None, code=N.LABEL_U8, lattice=None, out=other, out_label=None, ws=fake,
             ws_bytes=big, extent=(32, 32, 32)):
        return lib.ru3d_augment_patch_spatial(image, label, code, *extent, 1, ctypes.byref(pr) if pr else None,
                                              ctypes.byref(sp) if sp else None, lattice, None, out, out_label, ws,
                                              ws_bytes, None)

    def failed(rc, word):
        return rc < 0 and word in lib.ru3d_last_error()

    pr, sp = params()
    assert failed(call(pr, None), b"null spatial params")
    assert failed(call(None, sp), b"bad argument")
    assert failed(call(pr, sp, extent=(0, 32, 32)), b"bad argument")
    assert failed(call(pr, sp, out=None), b"image and out_image")
    assert failed(call(pr, sp, label=fake), b"label and out_label")
    assert failed(call(pr, sp, image=None, out=None), b"nothing to resample")
    assert failed(call(pr, sp, label=fake, out_label=other, code=5), b"label dtype")
    assert failed(call(pr, sp, ws_bytes=64), b"workspace too small")
    assert failed(call(*params(patch=(16, 0, 16))), b"empty patch")
    assert failed(call(*params(patch=(2048, 2048, 1024))), b"patch too large")
    sp.centre[1] = float("nan")
    assert failed(call(pr, sp), b"non-finite centre[1]")
    pr, sp = params()
    sp.matrix[5] = float("inf")
    assert failed(call(pr, sp), b"non-finite matrix[5]")
    assert failed(call(*params(lattice=(4, 4, 4), spacing=(16, 2, 16)), lattice=fake), b"spacing[1] = 2")
    assert failed(call(*params(lattice=(4, 0, 4), spacing=(16, 16, 16)), lattice=fake), b"lattice[1] = 0")
    assert failed(call(*params(lattice=(4, 4, 5), spacing=(16, 16, 16)), lattice=fake), b"lattice[2] = 5")
    assert failed(call(*params(lattice=(4, 4, 4), spacing=(16, 16, 16))), b"lattice pointer is null")
    assert failed(call(*params(patch=(5, 133, 249), lattice=(4, 36, 65), spacing=(4, 4, 4)), lattice=fake), b"LDS budget")
    assert failed(call(*params(patch=(5, 137, 245), lattice=(4, 37, 64), spacing=(4, 4, 4)), lattice=fake), b"LDS budget")
