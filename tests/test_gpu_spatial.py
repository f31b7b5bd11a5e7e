"""The free-form spatial transform of the on-device patch sampler (rotation, per-axis zoom, cubic B-spline elastic
deformation: spatial_kernel in csrc/augment.hip behind ru3d_augment_patch_spatial) against its numpy twin
`transform.RandomSpatialCrop` under one numpy seed.

Tolerances: image 2e-6 * max(1, max|image|) before the intensity chain (float64 coordinates and lerps rounded to float32
on both sides; the coordinate chain is summed in a different order, 1e-13 voxels apart) and 2e-5 after it (float32 mean
and powf).  Labels are identical except where the twin's decision margin (top class weight minus runner-up, float64) is
below 1e-9: those voxels are counted and the count must stay a handful.  Run with `-m gpu`."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no HIP device", allow_module_level=True)

import _native as N  # noqa: E402
import augment  # noqa: E402
import spatial  # noqa: E402
import transform as T  # noqa: E402

DEV = torch.device("cuda:0")
RUN_TRAIN = dict(scale=0.1, rotation=((-0.1 * np.pi, 0.1 * np.pi), (0, 0), (0, 0)), elastic_spacing=16,
                 elastic_magnitude=(0, 4))
INTENSITY = dict(contrast=[0.9, 1.1], brightness=[0.9, 1.1], gamma=[0.9, 1.1])
OFF = dict(contrast=None, brightness=None, gamma=None)


def _volume(shape, classes, dtype=np.uint8, channels=1, seed=0):
    rng = np.random.RandomState(seed)
    g = np.meshgrid(*[np.linspace(-1, 1, s, dtype=np.float32) for s in shape], indexing="ij")
    img = np.stack([(np.sin((4 + c) * g[0]) * np.cos(3 * g[1]) + g[2] ** 2 + 0.05 * rng.randn(*shape)) * (1 + 2 * c)
                    for c in range(channels)], axis=-1).astype(np.float32)
    lab = np.zeros(shape, dtype=dtype)
    lab[np.sqrt(g[0] ** 2 + (1.2 * g[1]) ** 2 + g[2] ** 2) < 0.8] = 1
    if classes > 2:
        lab[np.sqrt((g[0] - 0.2) ** 2 + g[1] ** 2 + g[2] ** 2) < 0.35] = 2
    if classes > 3:
        lab[np.sqrt((g[0] + 0.3) ** 2 + (g[1] - 0.1) ** 2 + g[2] ** 2) < 0.2] = 3
    return img, lab


def _twin(img, lab, seed, patch, mirror_p, intensity, **kw):
    """RandomSpatialCrop -> RandomMirror -> RandomContrast / Brightness / Gamma -> ToTensor with the margin carried
    along: (image before the intensity chain, image after it, label, margin)."""
    np.random.seed(seed)
    case = T.RandomSpatialCrop(crop_size=list(patch), label_margin=True, **kw)({"image": img.copy(), "label": lab.copy()})
    arrays = [case["image"], case["label"], case["label_margin"]]
    for axis, p in enumerate(mirror_p or ()):
        if np.random.uniform() < p:                                    # RandomMirror's draw
            arrays = [np.flip(a, axis).copy() for a in arrays]
    plain = after = arrays[0]
    for op, name in ((T.adjust_contrast, "contrast"), (T.adjust_brightness, "brightness"), (T.adjust_gamma, "gamma")):
        if intensity.get(name) is not None:
            after = op(after, np.random.uniform(*intensity[name]))    # _ImageFactor's draw
    return np.moveaxis(plain, -1, 0), np.moveaxis(after, -1, 0), arrays[1], arrays[2]


def _device(case, seed, patch, mirror_p, intensity, **kw):
    np.random.seed(seed)
    aug = augment.DeviceAugment(crop_size=list(patch), mirror_p=mirror_p, **intensity, **kw)
    img, lab = aug.sample(case)
    torch.cuda.synchronize()
    return img.cpu().numpy(), lab.cpu().numpy()


def _hold(img, lab, seed, patch, mirror_p=None, intensity=None, **kw):
    """Device against twin, before and after the intensity chain; returns the number of ambiguous label voxels."""
    case = augment.DeviceCase(img, lab, DEV)
    kw.setdefault("crop_mode", "random")
    want_plain, want_after, want_lab, margin = _twin(img, lab, seed, patch, mirror_p, intensity or OFF, **kw)
    got_plain, got_lab = _device(case, seed, patch, mirror_p, OFF, **kw)
    assert got_plain.shape == want_plain.shape and got_lab.dtype == np.int64
    assert np.abs(got_plain - want_plain).max() <= 2e-6 * max(1.0, np.abs(want_plain).max())
    differ = got_lab != want_lab.astype(np.int64)
    assert not (differ & (margin >= 1e-9)).any(), "labels differ where the twin's decision is not a tie"
    assert int(differ.sum()) <= 8, "%d label voxels sit on a tie" % int(differ.sum())
    assert np.ptp(got_plain) > 0                                              # not a patch of padding
    if intensity:
        got_after, lab2 = _device(case, seed, patch, mirror_p, intensity, **kw)
        assert np.array_equal(lab2, got_lab)
        assert np.abs(got_after - want_after).max() <= 2e-5 * max(1.0, np.abs(want_after).max())
    return int(differ.sum())


def test_run_train_recipe_on_its_own_patch():
    img, lab = _volume((200, 190, 100), 3)
    _hold(img, lab, 5, (160, 160, 80), mirror_p=(0.5, 0.5, 0.5), intensity=INTENSITY, **RUN_TRAIN)


def test_rotation_about_all_three_axes_at_128():
    img, lab = _volume((176, 160, 144), 4)
    _hold(img, lab, 42, (128, 128, 128), scale=0.1, rotation=0.3)


@pytest.mark.parametrize("spacing,patch", [(16, (128, 128, 128)), (32, (96, 80, 64)), ((4, 8, 16), (64, 48, 40))])
def test_elastic_only(spacing, patch):
    img, lab = _volume((150, 140, 136), 4, seed=3)
    _hold(img, lab, 9, patch, scale=0.1, elastic_spacing=spacing, elastic_magnitude=(6, 8))


@pytest.mark.parametrize("classes,dtype", [(2, np.int64), (4, np.int64), (2, np.uint8), (4, np.uint8)])
def test_everything_together_two_channels(classes, dtype):
    img, lab = _volume((100, 96, 90), classes, dtype, channels=2, seed=classes)
    _hold(img, lab, 17 + classes, (64, 72, 80), mirror_p=(0.9, 0.5, 0.9), intensity=INTENSITY, scale=0.2,
          rotation=((-0.2, 0.2), (-0.1, 0.3), (0.05, 0.25)), elastic_spacing=(16, 8, 16), elastic_magnitude=(2, 5),
          enforce_label_indices=[1], crop_margin=2)


@pytest.mark.parametrize("patch", [(37, 50, 65), (33, 47, 1), (1, 9, 70), (5, 1, 130)])
def test_extents_that_do_not_fill_a_workgroups_rows(patch):
    """8 rows of z per workgroup pass, 64 voxels of a row per wave pass: ragged in every direction, a row of one voxel
    (many row groups per workgroup: the partials have one slot per 256 voxels), a single row."""
    img, lab = _volume((80, 72, 90), 4, seed=8)
    _hold(img, lab, 3, patch, mirror_p=(0.5, 0.5, 0.5), intensity=INTENSITY, scale=0.1, rotation=0.2,
          elastic_spacing=(4, 8, 16), elastic_magnitude=(1, 3))


def test_crop_box_and_rotation_that_leave_the_volume():
    img, lab = _volume((60, 56, 50), 3, seed=4)
    kw = dict(scale=[0.6, 0.7], rotation=0.5, elastic_spacing=16, elastic_magnitude=(0, 6), image_pad_cval=-1.5,
              label_pad_cval=2, crop_mode="center")
    _hold(img, lab, 21, (64, 64, 64), **kw)
    case = augment.DeviceCase(img, lab, DEV)
    got, got_lab = _device(case, 21, (64, 64, 64), None, OFF, **kw)
    assert (got[0, 0, 0, :4] == -1.5).all() and (got_lab[0, 0, :4] == 2).all()    # a corner far outside the volume


def test_identity_parameters_equal_the_axis_aligned_entry_point():
    for classes, seed in ((2, 1), (4, 2)):
        img, lab = _volume((90, 84, 80), classes, seed=seed)
        case = augment.DeviceCase(img, lab, DEV)
        np.random.seed(seed)
        aug = augment.DeviceAugment(scale=0.15, crop_size=[64, 56, 72], crop_mode="random", crop_margin=-6)
        pr, mask, geometry = aug._draw(case)
        assert geometry is None
        centre, matrix = spatial.patch_geometry(list(pr.lo), list(pr.before), list(pr.patch))
        sp = N.SpatialParams()
        sp.centre[:], sp.matrix[:] = centre.tolist(), matrix.reshape(-1).tolist()
        a_img, a_lab = aug._launch(case, (pr, mask, None), None, None, None)
        b_img, b_lab = aug._launch(case, (pr, mask, (sp, None)), None, None, None)
        torch.cuda.synchronize()
        assert (a_img - b_img).abs().max().item() <= 1e-6 * max(1.0, a_img.abs().max().item())
        assert torch.equal(a_lab, b_lab)


def test_largest_accepted_lattice_and_the_first_refused_one():
    """(ny + 4) * nz <= 2560: a 5 x 133 x 245 patch at spacing 4 has 5 x 36 x 64 control points (40 * 64), 249 voxels
    along z make 65."""
    assert spatial.lattice_shape((5, 133, 245), (4, 4, 4)) == (4, 36, 64)
    img, lab = _volume((40, 150, 250), 4, seed=6)
    _hold(img, lab, 2, (5, 133, 245), scale=0.05, rotation=0.1, elastic_spacing=4, elastic_magnitude=(1, 2),
          crop_mode="center")
    with pytest.raises(ValueError, match="elastic_spacing"):
        augment.DeviceAugment(crop_size=[5, 133, 249], elastic_spacing=4, elastic_magnitude=(1, 2))
    # the C entry point refuses it too, before any launch
    case = augment.DeviceCase(img, lab, DEV)
    pr, sp = N.PatchParams(), N.SpatialParams()
    pr.patch[:], pr.before[:] = (5, 133, 249), (5, 133, 249)
    sp.matrix[:] = np.eye(3).reshape(-1).tolist()
    sp.lattice[:], sp.spacing[:] = (4, 36, 65), (4, 4, 4)
    lattice = torch.zeros(3 * 4 * 36 * 65, dtype=torch.float32, device=DEV)
    out = torch.full((1, 5, 133, 249), 7.0, dtype=torch.float32, device=DEV)
    ws = N.workspace(N.lib.ru3d_augment_workspace_bytes(5, 133, 249), DEV)
    N.note_device(DEV)
    rc = N.lib.ru3d_augment_patch_spatial(N.ptr(case.image), None, N.LABEL_U8, 40, 150, 250, 1, ctypes.byref(pr),
                                          ctypes.byref(sp), N.ptr(lattice), None, N.ptr(out), None, N.ptr(ws),
                                          ws.numel(), N.stream())
    assert rc < 0 and b"LDS budget" in N.lib.ru3d_last_error()
    torch.cuda.synchronize()
    assert (out == 7.0).all()


def test_batch_slices_sentinels_determinism_and_batch():
    cases = [augment.DeviceCase(*_volume((70, 66, 60), 4, channels=2, seed=s), DEV) for s in (1, 2)]
    kw = dict(scale=0.1, crop_size=[40, 36, 44], rotation=0.3, elastic_spacing=8, elastic_magnitude=(1, 4))
    x = torch.full((3, 2, 40, 36, 44), -77.0, dtype=torch.float32, device=DEV)
    y = torch.full((3, 40, 36, 44), -77, dtype=torch.int64, device=DEV)
    np.random.seed(5)
    augment.DeviceAugment(**kw).sample(cases[0], x[1], y[1])
    torch.cuda.synchronize()
    assert (x[0] == -77).all() and (x[2] == -77).all() and (y[0] == -77).all() and (y[2] == -77).all()
    assert (x[1] != -77).all() and int(y[1].min()) >= 0 and int(y[1].max()) <= 3
    np.random.seed(5)
    again, again_lab = augment.DeviceAugment(**kw).sample(cases[0])
    assert torch.equal(again, x[1]) and torch.equal(again_lab, y[1])               # two runs: the same bits
    # batch(): every lattice of the batch in one upload - the patches of the same draws made one by one
    np.random.seed(6)
    b = augment.DeviceAugment(**kw).batch(cases, 3)
    np.random.seed(6)
    one = augment.DeviceAugment(**kw)
    for i in range(3):
        img, lab = one.sample(cases[int(np.random.randint(0, 2))])
        assert torch.equal(b["image"][i], img) and torch.equal(b["label"][i], lab)
    assert not torch.equal(b["image"][0], b["image"][1])
    # rotation alone goes through batch() without a lattice
    np.random.seed(7)
    r = augment.DeviceAugment(scale=0.1, crop_size=[40, 36, 44], rotation=0.3).batch(cases, 2)
    assert tuple(r["image"].shape) == (2, 2, 40, 36, 44) and torch.isfinite(r["image"]).all()


def test_trainer_fit_epoch_with_the_spatial_keywords():
    import loss as L
    import network
    import trainer as TR

    class Cases(torch.utils.data.Dataset):
        def __init__(self):
            self.items = [dict(zip(("image", "label"), _volume((48, 44, 40), 2, seed=s))) for s in range(3)]

        def __len__(self):
            return len(self.items)

        def __getitem__(self, i):
            return dict(self.items[i])

    torch.manual_seed(0)
    np.random.seed(0)
    model = network.ResUnet3D(2, 8, 1, 2).to(DEV)
    aug = augment.DeviceAugment(scale=0.1, crop_size=32, rotation=((-0.1 * np.pi, 0.1 * np.pi), (0, 0), (0, 0)),
                                elastic_spacing=8, elastic_magnitude=(0, 3))
    seen = []

    def transform(case):
        out = aug(case)
        seen.append((int(out["label"].min()), int(out["label"].max()), tuple(out["image"].shape)))
        return out

    tr = TR.Trainer(model=model, optimizer=torch.optim.Adam(model.parameters(), lr=1e-4), loss=L.HybirdLoss(),
                    dataset=Cases(), batch_size=1, valid_split=0.0, dataloader_kwargs={"num_workers": 0},
                    metrics={"dice": L.Dice()}, train_transform=transform, progress=False)
    tr.fit(num_epochs=1)
    torch.cuda.synchronize()
    assert len(seen) == 3 and all(lo >= 0 and hi <= 1 and shape == (1, 32, 32, 32) for lo, hi, shape in seen)
    assert all(torch.isfinite(p).all() for p in model.parameters())
    logits = model(aug.batch([augment.DeviceCase(*_volume((48, 44, 40), 2), DEV)], 1)["image"])
    assert torch.isfinite(logits).all()
