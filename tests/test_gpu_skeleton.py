"""GPU checks of csrc/skeleton.hip and what is built on it: skeleton.thin voxel for voxel against the numpy twin that
defines it (word boundaries, padding bits, subfield parity, a solid that touches every face), the iteration count,
classify / length / overlap / radii against the numpy route with ==, transform.skeletonize on HIP tensors, the trainer's
centreline drivers on HIP operands against the host route, and the centreline PLY files."""
import numpy as np
import pytest
import scipy.ndimage as ndi
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no HIP device", allow_module_level=True)

import _native as N  # noqa: E402
import meshfile  # noqa: E402
import morphology  # noqa: E402
import nifti  # noqa: E402
import skeleton  # noqa: E402
import trainer  # noqa: E402
import transform  # noqa: E402
from test_host_skeleton import FIXTURES, blob, thinned, tree_case  # noqa: E402

SPACINGS = [(1.0, 1.0, 1.0), (0.75, 0.5, 3.0)]          # dyadic: the squared distances are exact whichever feature ties


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def upload(volume, dev):
    return torch.from_numpy(np.ascontiguousarray(volume)).to(dev)


def packed(volume, dev):
    return morphology.pack(upload(volume, dev))


def volume_of(mask):
    return morphology.unpack(mask).cpu().numpy().astype(bool)


def check_thin(volume, dev, want=None):
    """skeleton.thin of `volume` against the twin: voxels, iteration count, padding bits, the input left alone."""
    if want is None:
        want = transform._skeleton_numpy(volume.reshape((1,) * (3 - volume.ndim) + volume.shape))
    mask = packed(volume, dev)
    before = mask.bits.clone()
    skel, iterations = skeleton.thin(mask, return_iterations=True)
    assert torch.equal(mask.bits, before)
    assert skel.shape == volume.shape and (volume_of(skel) == want[0].reshape(volume.shape)).all()
    assert iterations == want[1]
    Z = volume.shape[-1]
    if Z & 63:
        assert int((skel.bits[..., -1] >> (Z & 63)).ne(0).sum().item()) == 0
    assert torch.equal(morphology.pack(morphology.unpack(skel)).bits, skel.bits)
    return skel


@pytest.mark.parametrize("Z", [1, 2, 63, 64, 65, 130])
def test_thin_across_word_boundaries(dev, Z):
    volume = ndi.binary_dilation(np.random.RandomState(Z).rand(7, 9, Z) < 0.04, iterations=2)
    assert volume.any()
    check_thin(volume, dev)


@pytest.mark.parametrize("shape", [(33, 18, 70), (16, 17, 128)])
def test_thin_random_blobs(dev, shape):
    volume = blob(sum(shape), shape)
    skel = check_thin(volume, dev)
    assert 0 < skeleton.overlap(skel, skel)[0] < int(volume.sum())


def test_thin_solid_that_touches_every_face(dev):
    check_thin(np.ones((9, 10, 67), dtype=bool), dev)
    check_thin(np.zeros((3, 4, 5), dtype=bool), dev)


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_thin_fixtures_and_their_translates(dev, name):
    volume, skel, iterations = thinned(name)
    check_thin(volume, dev, (skel, iterations))
    moved = np.zeros(tuple(s + 1 for s in volume.shape), dtype=bool)
    moved[1:, 1:, 1:] = volume                                              # every voxel changes its subfield
    check_thin(moved, dev)


def test_thin_fewer_axes_and_max_iterations(dev):
    plane = np.zeros((9, 12), dtype=bool)
    plane[2:7, 1:11] = True
    check_thin(plane, dev)
    check_thin(np.array([0, 1, 1, 1, 0, 1], dtype=bool), dev)
    volume = thinned('ball')[0]
    for limit in (0, 1, 2):
        want = transform._skeleton_numpy(volume, limit)
        skel, iterations = skeleton.thin(packed(volume, dev), limit, return_iterations=True)
        assert iterations == want[1] == limit and (volume_of(skel) == want[0]).all()
    with pytest.raises(ValueError):
        skeleton.thin(packed(volume, dev), -2)
    with pytest.raises(ValueError):
        skeleton.thin(upload(volume, dev))


@pytest.mark.parametrize("name", ["dilated_y", "shell", "blob"])
def test_classify_length_overlap_radii(dev, name):
    if name == "blob":
        volume = blob(7, (17, 19, 67))
        skel = transform._skeleton_numpy(volume)[0]
    else:
        volume, skel, _ = thinned(name)
    mask, thin = packed(volume, dev), packed(skel, dev)
    ends, junctions, n, n_ends, n_junctions = skeleton.classify(thin)
    want = transform._skeleton_classify_numpy(skel)
    assert (n, n_ends, n_junctions) == want[2:]
    assert (volume_of(ends) == want[0]).all() and (volume_of(junctions) == want[1]).all()
    # a mask that is not thin: every count from 0 to 26 occurs, the counter saturates
    _, _, n, n_ends, n_junctions = skeleton.classify(mask)
    assert (n, n_ends, n_junctions) == transform._skeleton_classify_numpy(volume)[2:]
    other = np.roll(volume, 2, axis=2)
    assert skeleton.overlap(thin, packed(other, dev)) == (int(skel.sum()), int(other.sum()), int((skel & other).sum()))
    for spacing in SPACINGS + [(0.7, 0.83, 3.1)]:
        assert skeleton.length(thin, spacing) == transform._skeleton_length_numpy(skel, spacing)
    assert skeleton.length(mask) == transform._skeleton_length_numpy(volume, (1.0, 1.0, 1.0))
    for spacing in SPACINGS:
        sq = skeleton.radii_squared(thin, mask, spacing).cpu().numpy()
        want_sq = trainer._radii_squared_numpy(skel, volume, spacing)
        assert sq.shape == want_sq.shape and (sq == want_sq).all()
        rooted = ndi.distance_transform_edt(volume, sampling=spacing)[skel]
        assert (sq == rooted * rooted).all() or np.allclose(np.sqrt(sq), rooted, rtol=4e-16, atol=0)
        assert skeleton.radii(thin, mask, spacing) == trainer._radius_stats_numpy(want_sq)[1:]
    empty = packed(np.zeros_like(volume), dev)
    assert skeleton.classify(empty)[2:] == (0, 0, 0) and skeleton.length(empty) == 0.0
    assert all(np.isnan(v) for v in skeleton.radii(empty, mask))


def test_thin_classify_length_overlap_with_a_capped_grid(dev):
    """The word loops (sk_mark of every thinning pass, classify, the pair counts of length, overlap) cap their grid at 8
    blocks a CU of the budget.  (136, 128, 64): 136 * 128 * 1 = 17408 words = 68 blocks of 256 threads uncapped, under the
    2048 of the whole chip; under a budget of 8 CUs the cap is 64, so 1024 words are done on the loop's second trip.  The
    equalities are those of check_thin and test_classify_length_overlap_radii."""
    volume = blob(11, (136, 128, 64))
    want = transform._skeleton_numpy(volume)
    try:
        assert N.lib.ru3d_set_cu_budget(8) == 0
        thin = check_thin(volume, dev, want)
        mask = packed(volume, dev)
        for m, v in ((thin, want[0]), (mask, volume)):
            ends, junctions, n, n_ends, n_junctions = skeleton.classify(m)
            ref = transform._skeleton_classify_numpy(v)
            assert (n, n_ends, n_junctions) == ref[2:]
            assert (volume_of(ends) == ref[0]).all() and (volume_of(junctions) == ref[1]).all()
        other = np.roll(volume, 2, axis=2)
        assert skeleton.overlap(thin, packed(other, dev)) == (int(want[0].sum()), int(other.sum()), int((want[0] & other).sum()))
        for spacing in SPACINGS:
            assert skeleton.length(thin, spacing) == transform._skeleton_length_numpy(want[0], spacing)
    finally:
        N.lib.ru3d_set_cu_budget(0)
    assert N.lib.ru3d_get_cu_budget() == torch.cuda.get_device_properties(dev).multi_processor_count


def test_complement_keeps_the_padding_clear(dev):
    volume = blob(3, (5, 6, 70))
    got = skeleton.complement(packed(volume, dev))
    assert torch.equal(got.bits, packed(~volume, dev).bits)


def test_skeletonize_on_hip_tensors(dev):
    volume = thinned('dilated_y')[0]
    for array in (volume, volume.astype(np.uint8) * 5):
        got = transform.skeletonize(upload(array, dev))
        want = transform.skeletonize(array)
        assert got.is_cuda and got.dtype == upload(array, dev).dtype and (got.cpu().numpy() == want).all()
    got = transform.skeletonize(upload(volume, dev), max_iterations=1)
    assert (got.cpu().numpy() == transform.skeletonize(volume, max_iterations=1)).all()
    labels = volume.astype(np.uint8) * 2
    case = transform.Skeletonize(label=2)({'pred': upload(labels, dev)})
    assert case['pred'].is_cuda and (case['pred'].cpu().numpy() == transform.Skeletonize(label=2)({'pred': labels})['pred']).all()


def same_dicts(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.keys() == w.keys()
        for k in g:
            if isinstance(w[k], np.ndarray):
                assert g[k].shape == w[k].shape and (g[k] == w[k]).all(), k
            else:
                assert g[k] == w[k] or (g[k] != g[k] and w[k] != w[k]), k


def test_centerline_drivers_on_hip_operands(dev, tmp_path):
    case = tree_case()
    case['pred'][2:5, 2:5, 2:9] = 2                                         # a second structure the label does not have
    affine = np.diag([0.75, 0.5, 3.0, 1.0])
    affine[:3, 3] = (-20.0, 4.0, 100.0)
    on_device = {k: upload(v, dev) for k, v in case.items()}
    same_dicts(trainer.evaluate_centerline_case(on_device), trainer.evaluate_centerline_case(case))
    same_dicts(trainer.evaluate_centerline_case({'pred': on_device['pred'], 'label': case['label']}, labels=[1, 2, (1, 2)]),
               trainer.evaluate_centerline_case(case, labels=[1, 2, (1, 2)]))
    want = trainer.centerline_case({'pred': case['pred'], 'affine': affine})
    assert [r['label'] for r in want] == [1, 2] and want[0]['ends'] == 2
    same_dicts(trainer.centerline_case({'pred': on_device['pred'], 'affine': affine}), want)
    lean = trainer.centerline_case({'pred': on_device['pred'], 'affine': affine}, return_device=True)
    same_dicts(lean, [{k: v for k, v in r.items() if k not in ('points', 'radii')} for r in want])

    for kind in ('label', 'pred'):
        (tmp_path / kind).mkdir()
        nifti.save(case[kind], affine, tmp_path / kind / 'case_0.nii.gz')
    results = trainer.batch_extract_centerline(tmp_path / 'pred', tmp_path / 'out', device=dev)
    assert len(results) == 1 and len(results[0]) == 2
    for r, w in zip(results[0], want):
        points, radius = meshfile.read_points_ply(r['file'])
        assert (points == w['points']).all() and (radius == w['radii']).all()
        assert (points == r['points']).all() and (radius == r['radii']).all()
    same_dicts(trainer.evaluate_centerline(tmp_path / 'label' / 'case_0.nii.gz', tmp_path / 'pred' / 'case_0.nii.gz', dev),
               trainer.evaluate_centerline_case(case))
