"""Gaussian noise, Gaussian blur and simulated low resolution in the on-device patch sampler (csrc/degrade.hip behind
ru3d_augment_degrade, DeviceAugment(noise=..., blur=..., low_res=...)) against the numpy twins of module `degrade`.

Bounds (every voxel compared): noise 2^-23 * max|out| (float64 transcendentals on both sides, one float32 rounding);
blur 3 * 2^-23 * max|x| (three stored passes, each at most one float32 step apart; convex weights do not amplify);
low-res 2^-23 * max|x|, and the input bits at zoom 1.  Full chain against the twin Compose under one numpy seed: labels
identical, image within 2e-5 (what test_gpu_augment.py allows the intensity chain) + 1.4 * the three stage bounds (the
chain's gain is at most 1.1^3).  Run with `-m gpu`."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no HIP device", allow_module_level=True)

import augment  # noqa: E402
import degrade  # noqa: E402
import transform as T  # noqa: E402

DEV = torch.device("cuda:0")
EPS = 2.0 ** -23
OFF = dict(contrast=None, brightness=None, gamma=None)
SHAPES = {"odd": ((19, 33, 70), 2), "cube": ((64, 64, 64), 1), "thin": ((5, 33, 70), 2)}
DRAWS = {"noise": 4, "blur": 2, "low_res": 2}          # u and the parameters, when the op applies


class Recorder:
    """Hands out the draws of a numpy RandomState and keeps them."""

    def __init__(self, seed):
        self.state, self.values = np.random.RandomState(seed), []

    def uniform(self, *args, **kw):
        self.values.append(self.state.uniform(*args, **kw))                      # size=: the elastic lattice, one array
        return self.values[-1]

    def randint(self, *args, **kw):
        self.values.append(self.state.randint(*args, **kw))
        return self.values[-1]


class Script:
    """Replays recorded draws; a call beyond the list fails."""

    def __init__(self, values):
        self.values = list(values)

    def _next(self, *args, **kw):
        assert self.values, "a draw the script does not foresee"
        return self.values.pop(0)

    uniform = randint = _next


_CASES = {}


def _case(tag):
    """A case about 1.3 times the patch, standard-normal scale (smooth structure plus voxel noise), four classes."""
    if tag not in _CASES:
        patch, channels = SHAPES[tag]
        shape = tuple(int(round(1.3 * p)) for p in patch)
        rng = np.random.RandomState(len(tag))
        g = np.meshgrid(*[np.linspace(-1, 1, s) for s in shape], indexing="ij")
        img = np.stack([np.sin((3 + c) * g[0]) * np.cos(4 * g[1] + c) + g[2] + 0.5 * rng.randn(*shape)
                        for c in range(channels)], axis=-1)
        img = ((img - img.mean()) / img.std()).astype(np.float32)
        lab = np.zeros(shape, dtype=np.uint8)
        lab[np.sqrt(g[0] ** 2 + (1.2 * g[1]) ** 2 + g[2] ** 2) < 0.8] = 1
        lab[np.sqrt((g[0] - 0.2) ** 2 + g[1] ** 2 + g[2] ** 2) < 0.35] = 2
        lab[np.sqrt((g[0] + 0.3) ** 2 + (g[1] - 0.1) ** 2 + g[2] ** 2) < 0.2] = 3
        _CASES[tag] = (img, lab, augment.DeviceCase(img, lab, DEV))
    return _CASES[tag]


def _one_op(tag, name, value, seed=3):
    """The op alone, forced (p = 1, a range of one value), behind the axis-aligned resampler with the intensity chain off
    -> (the resampled patch it ran on, the device's result, the drawn parameters)."""
    patch, _ = SHAPES[tag]
    case = _case(tag)[2]
    kw = dict(scale=0.1, crop_size=list(patch), crop_mode="random", **OFF)
    rec = Recorder(seed)
    got, got_lab = augment.DeviceAugment(rng=rec, **kw, **{name: (1.0, (value, value))}).sample(case)
    base = Script(rec.values[:-DRAWS[name]])
    plain, plain_lab = augment.DeviceAugment(rng=base, **kw).sample(case)
    torch.cuda.synchronize()
    assert not base.values and torch.equal(got_lab, plain_lab)                  # labels are untouched
    return plain.cpu().numpy(), got.cpu().numpy(), rec.values[-DRAWS[name] + 1:]


def _report(what, got, want, bound):
    err = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
    print("%s: max error %.3g, bound %.3g" % (what, err, bound))
    return err


@pytest.mark.parametrize("tag", ["odd", "cube"])
def test_noise_alone(tag):
    plain, got, (variance, k0, k1) = _one_op(tag, "noise", 0.07)
    assert variance == 0.07
    want = degrade.gaussian_noise(plain, variance, (k0, k1))
    assert got.shape == want.shape and got.dtype == np.float32
    assert _report("noise " + tag, got, want, EPS * np.abs(want).max()) <= EPS * np.abs(want).max()
    field = (got.astype(np.float64) - plain).ravel() / np.sqrt(variance)
    assert abs(field.mean()) <= 4.0 / np.sqrt(field.size) and abs(field.var() - 1.0) <= 0.05


@pytest.mark.parametrize("tag,sigma,radius", [("cube", 0.5, 2), ("cube", 1.5, 6), ("cube", 4.0, 16), ("odd", 1.5, 6),
                                              ("thin", 1.0, 4)])
def test_blur_alone(tag, sigma, radius):
    assert degrade.blur_radius(sigma) == radius
    plain, got, (drawn,) = _one_op(tag, "blur", sigma)
    assert drawn == sigma
    want = degrade.gaussian_blur(plain, sigma)
    bound = 3 * EPS * np.abs(plain).max()
    assert _report("blur %s sigma %g" % (tag, sigma), got, want, bound) <= bound
    assert np.abs(got - plain).max() > 0.05                                      # it did blur


@pytest.mark.parametrize("tag", ["odd", "cube"])
@pytest.mark.parametrize("zoom", [0.5, 1.0])
def test_low_resolution_alone(tag, zoom):
    plain, got, (drawn,) = _one_op(tag, "low_res", zoom)
    assert drawn == zoom
    want = degrade.simulate_low_resolution(plain, zoom)
    bound = EPS * np.abs(plain).max()
    assert _report("low-res %s zoom %g" % (tag, zoom), got, want, bound) <= bound
    if zoom == 1.0:
        assert np.array_equal(got, plain)                                        # the input bits
    else:
        assert np.abs(got - plain).max() > 0.05


@pytest.mark.parametrize("resampler", ["plain", "spatial"])
@pytest.mark.parametrize("tag", ["odd", "cube"])
def test_full_chain_against_the_twin_compose(tag, resampler):
    patch, _ = SHAPES[tag]
    img, lab, case = _case(tag)
    seen = []

    def note(c):
        seen.append(float(np.abs(c["image"]).max()))
        return c

    ops = dict(noise=(1.0, (0.02, 0.1)), blur=(1.0, (0.5, 1.0)), low_res=(1.0, (0.5, 1.0)))
    intensity = dict(contrast=[0.9, 1.1], brightness=[0.9, 1.1], gamma=[0.9, 1.1])
    crop = dict(scale=0.1, crop_size=list(patch), crop_mode="random")
    if resampler == "spatial":
        crop.update(rotation=0.2, elastic_spacing=8, elastic_magnitude=(1, 3))
        first = T.RandomSpatialCrop(**crop)
        source_lab = (lab > 0).astype(np.uint8)          # two classes: the label rule that interpolates and truncates
        case = augment.DeviceCase(img, source_lab, DEV)
    else:
        first = T.RandomRescaleCrop(**crop)
        source_lab = lab
    twin = T.Compose([first, T.RandomMirror((0.5, 0.5, 0.5)), T.RandomGaussianNoise(*ops["noise"]), note,
                      T.RandomGaussianBlur(*ops["blur"]), note, T.RandomLowResolution(*ops["low_res"]),
                      T.RandomContrast(intensity["contrast"]), T.RandomBrightness(intensity["brightness"]),
                      T.RandomGamma(intensity["gamma"]), T.ToTensor()])
    np.random.seed(23)
    want = twin({"image": img.copy(), "label": source_lab.copy()})
    np.random.seed(23)
    got, got_lab = augment.DeviceAugment(mirror_p=(0.5, 0.5, 0.5), **crop, **ops, **intensity).sample(case)
    torch.cuda.synchronize()
    assert np.array_equal(got_lab.cpu().numpy(), want["label"].astype(np.int64))
    after_noise, after_blur = seen
    bound = 2e-5 + 1.4 * (EPS * after_noise + 3 * EPS * after_noise + EPS * after_blur)
    assert _report("chain %s %s" % (tag, resampler), got.cpu().numpy(), want["image"], bound) <= bound


@pytest.mark.parametrize("resampler", ["plain", "spatial"])
def test_probability_zero_is_the_sampler_without_the_keywords(resampler):
    patch, _ = SHAPES["odd"]
    case = _case("odd")[2]
    kw = dict(scale=0.1, crop_size=list(patch), crop_mode="random")
    if resampler == "spatial":
        kw.update(rotation=0.2, elastic_spacing=8, elastic_magnitude=(1, 3))
    rec = Recorder(5)
    a, a_lab = augment.DeviceAugment(rng=rec, noise=(0.0, (0, 0.1)), blur=(0.0, (0.5, 1.0)), low_res=(0.0, (0.5, 1.0)),
                                     **kw).sample(case)
    values = rec.values[:-6] + rec.values[-3:]            # without the three u of the ops, in front of the intensity draws
    script = Script(values)
    b, b_lab = augment.DeviceAugment(rng=script, **kw).sample(case)
    torch.cuda.synchronize()
    assert not script.values and torch.equal(a, b) and torch.equal(a_lab, b_lab)


@pytest.mark.parametrize("resampler", ["plain", "spatial"])
def test_batch_equals_per_sample_calls(resampler):
    cases = [_case("odd")[2], augment.DeviceCase(_case("odd")[0][::-1].copy(), _case("odd")[1][::-1].copy(), DEV)]
    kw = dict(scale=0.1, crop_size=list(SHAPES["odd"][0]), crop_mode="random", noise=(1.0, (0.02, 0.1)),
              blur=(0.5, (0.5, 1.0)), low_res=(0.5, (0.5, 1.0)))
    if resampler == "spatial":
        kw.update(rotation=0.2, elastic_spacing=8, elastic_magnitude=(1, 3))
    rec = Recorder(9)
    batch = augment.DeviceAugment(rng=rec, **kw).batch(cases, 4)
    assert tuple(batch["image"].shape) == (4, 2, 19, 33, 70) and tuple(batch["label"].shape) == (4, 19, 33, 70)
    script = Script(rec.values)
    one = augment.DeviceAugment(rng=script, **kw)
    applied = set()
    for b in range(4):
        picked = cases[int(script.randint(0, 2))]
        drawn = one._draw(picked)
        applied.add((drawn[3].do_blur, drawn[3].do_low_res))
        lattice = augment._upload([drawn[2][1]], DEV)[0] if resampler == "spatial" else None
        img, lab = one._launch(picked, drawn, lattice, None, None)
        assert torch.isfinite(batch["image"][b]).all()
        assert torch.equal(batch["image"][b], img) and torch.equal(batch["label"][b], lab)
    torch.cuda.synchronize()
    assert not script.values and len(applied) > 1         # the batch mixed patches with and without blur / low-res
    assert not torch.equal(batch["image"][0], batch["image"][1])


def test_transform_functions_take_hip_tensors():
    """gaussian_noise / gaussian_blur / simulate_low_resolution on a channels-last HIP tensor: the device route."""
    img = _case("odd")[0][:19, :33, :70]
    dev = torch.from_numpy(img).to(DEV)
    for fn, args in ((T.gaussian_noise, (0.05, (3, 4))), (T.gaussian_blur, (0.9,)), (T.simulate_low_resolution, (0.6,))):
        got = fn(dev, *args)
        want = fn(img, *args)
        assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == img.shape
        assert np.abs(got.cpu().numpy() - want).max() <= 3 * EPS * max(np.abs(img).max(), np.abs(want).max())
    assert torch.equal(dev, torch.from_numpy(img).to(DEV))                       # the input is left alone
    with pytest.raises(Exception, match="radius"):
        T.gaussian_blur(dev[:5], 1.5)                                            # radius 6 on an extent of 5
