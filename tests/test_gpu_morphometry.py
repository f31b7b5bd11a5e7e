"""The morphometry kernels (csrc/morphometry.hip) against the numpy route of `morphometry`: the integer tables bit for
bit, the float64 minima / maxima to the rounding of one short sum, on shapes that take every path - the direct LDS table
and the hashed one, 16-byte loads and unaligned operands, uint8 classes and int32 components, one giant component and
thousands of small ones - and the memory contract of every entry point through the C ABI itself."""
import ctypes
import functools

import numpy as np
import pytest
import scipy.ndimage as ndi
import torch

import _native as N
import morphometry as M
import trainer as T

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
OBLIQUE = np.eye(4)
OBLIQUE[:3, :3] = np.array([[0.78, -0.21, 0.35], [0.16, 0.79, 0.62], [-0.09, 0.05, 2.91]])
OBLIQUE[:3, 3] = (12.5, -40.0, 7.25)
GRAM = M.gram(OBLIQUE)


def dev():
    return torch.device("cuda:0")


def blobs(shape, seed=0):
    rng = np.random.RandomState(seed)
    field = ndi.gaussian_filter(rng.rand(*shape), 1.5)
    return np.digitize(field, np.quantile(field, [0.4, 0.65, 0.85])).astype(np.uint8)


def speckle(density):
    rng = np.random.RandomState(int(density * 100))
    mask = rng.rand(40, 72, 130) < density
    labels, count = ndi.label(mask)
    return labels.astype(np.int32), count, mask.astype(np.uint8)


def line(n, axis):
    """ids 1, 2, 3 in stretches along one axis, a gap of background, a single voxel of id 4 where there is room"""
    v = np.zeros(n, dtype=np.uint8)
    v[:] = (np.arange(n) * 3 // n + 1)
    if n > 8:
        v[n // 2:n // 2 + 3] = 0
        v[n // 2 + 1] = 4
    shape = [1, 1, 1]
    shape[axis] = n
    return v.reshape(shape)


@functools.lru_cache(maxsize=None)
def case(name):
    """(ids, count, other or None, num_other): numpy operands, made once"""
    if name == "classes":                       # classes 0 .. 3 and a stray 255; id 4 has no voxel
        v = blobs((9, 10, 67))
        v[4, 5, 30:33] = 255
        return v, 4, None, 0
    if name == "ones":                          # one id that touches all six borders; Szz above 2^32 in one chunk
        return np.ones((2, 3, 1500), np.uint8), 1, None, 0
    if name == "speckle":                       # thousands of ids, many of one voxel: the hashed tables
        labels, count, mask = speckle(0.3)
        assert count > 2048
        return labels, count, mask, 2
    if name == "giant":                         # one component that holds nearly everything, beside small ones
        labels, count, mask = speckle(0.9)
        assert np.bincount(labels.ravel())[1:].max() > 0.8 * labels.size
        return labels, count, mask, 2
    if name == "giant_hashed":                  # the same volume with room for 3000 ids: the giant meets the hashed tables
        labels, count, mask, M_ = case("giant")
        return labels, 3000, mask, M_
    if name == "row":
        return line(300, 2), 5, None, 0
    if name == "column":
        return line(5, 0), 3, None, 0
    if name == "nothing":                       # count = 0
        return blobs((9, 10, 67)), 0, None, 0
    raise KeyError(name)


CASES = ("classes", "ones", "speckle", "giant", "giant_hashed", "row", "column", "nothing")


def frames_of(name):
    _, count, _, _ = case(name)
    rng = np.random.RandomState(count + 5)
    f = rng.normal(size=(count, 3, 4))
    f[:, 0, :] = (1.0, 0.0, 0.0, 0.0)           # an index axis itself: exact
    return f


@functools.lru_cache(maxsize=None)
def host(name):
    v, count, other, M_ = case(name)
    cand, starts, counts = M.candidates(v, count)
    d2, pair = M.feret(v, count, GRAM)
    return {'moments': M.moments(v, count), 'faces': M.faces(v, count, other, M_),
            'extents': M.extents(v, count, frames_of(name)), 'cand': cand, 'starts': starts, 'counts': counts,
            'd2': d2, 'pair': pair}


def upload(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def device(name):
    v, count, other, M_ = case(name)
    ids, oth = upload(v), upload(other)
    cand, starts, counts = M.candidates(ids, count)
    d2, pair = M.feret(ids, count, GRAM)
    out = {'moments': M.moments(ids, count), 'faces': M.faces(ids, count, oth, M_),
           'extents': M.extents(ids, count, frames_of(name)), 'cand': cand, 'starts': starts, 'counts': counts,
           'd2': d2, 'pair': pair}
    assert all(t.is_cuda for t in out.values())
    return {k: t.cpu().numpy() for k, t in out.items()}


def extent_tolerance(name):
    """4 u (|ax x| + |ay y| + |az z| + |b|), the largest over the id's voxels: the rounding of a four-term sum"""
    v, count, _, _ = case(name)
    f = np.abs(frames_of(name))
    tol = np.zeros((count, 3))
    lin, k = M._valid(v.reshape(M._check_shape(v.shape, "test")), count)
    if lin.size:
        x, y, z = (c.astype(np.float64)[:, None] for c in M._xyz(lin, M._check_shape(v.shape, "test")))
        fk = f[k - 1]
        np.maximum.at(tol, k - 1, fk[:, :, 0] * x + fk[:, :, 1] * y + fk[:, :, 2] * z + fk[:, :, 3])
    return 4 * U * tol


def sorted_groups(cand, starts, counts):
    return [np.sort(cand[s:s + c]) for s, c in zip(starts.tolist(), counts.tolist())]


def check_against_host(name, got):
    v, count, _, _ = case(name)
    want = host(name)
    assert got['moments'].dtype == np.int64 and np.array_equal(got['moments'], want['moments'])
    assert got['faces'].dtype == np.int64 and np.array_equal(got['faces'], want['faces'])
    tol = extent_tolerance(name)
    finite = np.isfinite(want['extents'])
    assert np.array_equal(np.isfinite(got['extents']), finite)
    assert np.array_equal(got['extents'][~finite], want['extents'][~finite])           # (+inf, -inf) of an empty id
    err = np.abs(np.where(finite, got['extents'], 0.0) - np.where(finite, want['extents'], 0.0))
    print("%s: extents worst error / bound %.3g" % (name, (err / np.maximum(tol[:, :, None], 1e-300)).max() if count else 0))
    assert np.all(err <= tol[:, :, None])
    assert np.array_equal(got['extents'][:, 0], want['extents'][:, 0])                  # the pure index axis: exact
    # candidates: the counted prefix, group by group (the order inside a group is not defined)
    assert np.array_equal(got['counts'], want['counts']) and np.array_equal(got['starts'], want['starts'])
    assert len(got['cand']) == int(want['counts'].sum())
    for a, b in zip(sorted_groups(got['cand'], got['starts'], got['counts']),
                    sorted_groups(want['cand'], want['starts'], want['counts'])):
        assert np.array_equal(a, b)
    # Feret: d^2 to the rounding of the sum, and a pair of voxels of the id that reproduces it
    d2, ref = got['d2'], want['d2']
    assert np.array_equal(d2 < 0, ref < 0) and np.array_equal(d2[ref < 0], ref[ref < 0])
    worst = np.abs(d2 - ref) / np.maximum(ref, 1e-300)
    print("%s: feret worst |d2 - ref| / d2 = %.3g u" % (name, (worst[ref > 0].max() / U) if (ref > 0).any() else 0))
    assert np.all(np.abs(d2 - ref) <= 8 * U * np.abs(ref))
    pair = got['pair']
    flat = v.reshape(M._check_shape(v.shape, "test"))
    for k in range(count):
        if ref[k] < 0:
            assert pair[k].tolist() == [-1] * 6
            continue
        p, q = pair[k, :3], pair[k, 3:]
        assert flat[tuple(p)] == k + 1 and flat[tuple(q)] == k + 1
    have = ref >= 0
    back = M.dist2(GRAM, (pair[have, :3] - pair[have, 3:]).astype(np.int64))
    assert np.all(np.abs(back - d2[have]) <= 8 * U * np.abs(d2[have]))
    single = want['moments'][:, 0] == 1
    assert np.all(d2[single] == 0.0) and np.array_equal(pair[single, :3], pair[single, 3:])


@pytest.mark.parametrize("name", CASES)
def test_device_tables_equal_the_numpy_route(name):
    first = device(name)
    check_against_host(name, first)
    second = device(name)                                                               # two runs: the same bits
    for key in ('moments', 'faces', 'extents', 'counts', 'd2', 'pair'):
        assert first[key].tobytes() == second[key].tobytes(), key


def test_the_cases_hold_what_they_are_for():
    m = host("speckle")['moments'][:, 0]
    assert len(m) > 2048 and (m == 1).sum() > 100 and (m > 0).all()
    assert host("classes")['moments'][3, 0] == 0 and host("classes")['d2'][3] == -1.0     # an id with no voxel
    v, _, _, _ = case("giant")
    big = int(np.argmax(host("giant")['moments'][:, 0]))
    xs, ys, zs = np.nonzero(v == big + 1)
    assert (xs.min(), ys.min(), zs.min()) == (0, 0, 0) and (xs.max(), ys.max(), zs.max()) == (39, 71, 129)
    assert host("ones")['moments'][0, 6] == 6743251500
    assert host("ones")['faces'][0, 2].tolist() == [2 * 3 * 1500, 2 * 2 * 1500, 2 * 2 * 3]


# ------------------------------------------------------------------------------------------------ the C ABI itself
class Arena:
    """One byte tensor filled with `fill`; operands and outputs are carved out of it with untouched bytes between"""

    def __init__(self, nbytes, fill):
        self.fill = fill
        self.buf = torch.full((nbytes,), fill, dtype=torch.uint8, device=dev())
        self.at = 64
        self.used = []

    def carve(self, nbytes, dtype=torch.uint8, skew=0):
        """a region of `nbytes` at 16 k + skew bytes"""
        start = (self.at + 15) // 16 * 16 + skew
        self.at = start + nbytes + 48
        assert self.at + 64 <= self.buf.numel()
        self.used.append((start, nbytes))
        return self.buf[start:start + nbytes].view(dtype)

    def put(self, array, skew=0):
        t = torch.from_numpy(np.ascontiguousarray(array)).to(dev())
        region = self.carve(t.numel() * t.element_size(), t.dtype, skew)
        region.copy_(t.reshape(-1))
        return region

    def untouched(self):
        keep = torch.ones(self.buf.numel(), dtype=torch.bool, device=dev())
        for start, nbytes in self.used:
            keep[start:start + nbytes] = False
        return bool((self.buf[keep] == self.fill).all())


def raw_tables(name, fill):
    """every entry point through N.lib, operands at addresses that are no multiple of 16, outputs in the arena"""
    v, count, other, M_ = case(name)
    X, Y, Z = M._check_shape(v.shape, "test")
    if other is None:
        other, M_ = v, count + 1
    idb = v.dtype.itemsize
    want = host(name)
    total = int(want['counts'].sum())
    capacity = total + 7
    arena = Arena(v.nbytes + other.nbytes + count * (80 + (M_ + 1) * 24 + 96 + 48 + 3 * 8 + 8 + 24) + capacity * 16 + 4096,
                  fill)
    ids = arena.put(v, skew=idb)                        # uint8 at 16 k + 1, int32 at 16 k + 4: the loads that are not 16 bytes
    oth = arena.put(other, skew=3)
    frames = arena.put(frames_of(name))
    out = {'moments': arena.carve(count * 80, torch.int64), 'faces': arena.carve(count * (M_ + 1) * 24, torch.int64),
           'extents': arena.carve(count * 48, torch.float64), 'counts': arena.carve(count * 8, torch.int64),
           'filled': arena.carve(count * 8, torch.int64), 'cand': arena.carve(capacity * 4, torch.int32),
           'row_d2': arena.carve(capacity * 8, torch.float64), 'row_partner': arena.carve(capacity * 4, torch.int32),
           'd2': arena.carve(count * 8, torch.float64), 'pair': arena.carve(count * 24, torch.int32)}
    starts = arena.put(want['starts'])
    p, s = N.ptr, N.stream(dev())
    lib = N.lib
    N.check(lib.ru3d_label_moments(p(ids), idb, X, Y, Z, count, p(out['moments']), s), "label_moments")
    N.check(lib.ru3d_label_faces(p(ids), idb, p(oth), M_, X, Y, Z, count, p(out['faces']), s), "label_faces")
    N.check(lib.ru3d_label_extents(p(ids), idb, X, Y, Z, count, p(frames), p(out['extents']), s), "label_extents")
    N.check(lib.ru3d_label_feret_count(p(ids), idb, X, Y, Z, count, p(out['counts']), s), "label_feret_count")
    N.check(lib.ru3d_label_feret_fill(p(ids), idb, X, Y, Z, count, p(starts), p(out['filled']), p(out['cand']), capacity, s),
            "label_feret_fill")
    N.check(lib.ru3d_label_feret(p(ids), idb, X, Y, Z, count, p(out['cand']), total, p(starts), p(out['counts']),
                                 (ctypes.c_double * 6)(*GRAM), p(out['row_d2']), p(out['row_partner']), p(out['d2']),
                                 p(out['pair']), s), "label_feret")
    torch.cuda.synchronize()
    assert arena.untouched(), "%s: bytes outside the operands and outputs changed" % name
    assert torch.equal(ids.cpu(), torch.from_numpy(v.reshape(-1))) and torch.equal(starts.cpu(), torch.from_numpy(want['starts']))
    got = {k: t.cpu().numpy() for k, t in out.items()}
    # behind the counted prefix the capacity buffers are as they were
    for key in ('cand', 'row_d2', 'row_partner'):
        tail = got[key][total:].view(np.uint8)
        assert np.all(tail == fill), key
        got[key] = got[key][:total]
    assert np.array_equal(got['filled'], got['counts'])
    got.update(moments=got['moments'].reshape(count, 10), faces=got['faces'].reshape(count, M_ + 1, 3),
               extents=got['extents'].reshape(count, 3, 2), pair=got['pair'].reshape(count, 6), starts=want['starts'])
    return got


@pytest.mark.parametrize("name", ("classes", "speckle", "giant", "giant_hashed", "row"))
def test_entry_points_write_their_outputs_and_nothing_else(name):
    guarded = raw_tables(name, 0xA5)
    check_against_host(name, guarded)
    prefilled = raw_tables(name, 0xFF)                                                  # what the outputs held does not matter
    for key in ('moments', 'faces', 'extents', 'counts', 'd2', 'pair'):
        assert guarded[key].tobytes() == prefilled[key].tobytes(), key
    assert [g.tolist() for g in sorted_groups(guarded['cand'], guarded['starts'], guarded['counts'])] == \
        [g.tolist() for g in sorted_groups(prefilled['cand'], prefilled['starts'], prefilled['counts'])]


# ------------------------------------------------------------------------------------------------ the report
def same_report(got, want, path=""):
    """field by field: integers, strings and the host arithmetic on exact tables equal, the two float64 searches to
    their rounding"""
    assert type(got) is type(want), path
    if isinstance(want, dict):
        assert list(got) == list(want), path
        for key in want:
            same_report(got[key], want[key], "%s.%s" % (path, key))
    elif isinstance(want, (list, tuple)):
        assert len(got) == len(want), path
        for i, (g, w) in enumerate(zip(got, want)):
            same_report(g, w, "%s[%d]" % (path, i))
    elif isinstance(want, float) and path.endswith("feret_mm"):
        assert got == pytest.approx(want, rel=8 * U), path                              # the root of d^2 within 8 u
    elif isinstance(want, float) and ".extents_mm" in path:
        # two ends, each a four-term sum of magnitudes below 500 mm here (the offset of the frame included), on the
        # device and in numpy: 2 * 2 * 4 u * 500
        assert got == pytest.approx(want, rel=0, abs=8000 * U), path
    else:
        assert got == want or (want != want and got != got), path


def test_describe_and_measure_case_equal_the_numpy_route():
    v = case("classes")[0]
    want = M.describe(v, 3, affine=OBLIQUE)
    got = M.describe(upload(v), 3, affine=OBLIQUE)
    same_report(got, want)
    options = dict(labels=[1, (2, 3)], gaps=[(1, 3)])
    numpy_case = {'case_id': 'c', 'pred': v, 'affine': OBLIQUE}
    hip_case = {'case_id': 'c', 'pred': upload(v), 'affine': OBLIQUE}
    same_report(T.measure_case(hip_case, **options), T.measure_case(numpy_case, **options))
    everything = T.measure_case(hip_case)                                               # labels=None: the values it holds
    assert [d['label'] for d in everything['structures']] == [1, 2, 3, 255]
    same_report(everything, T.measure_case(numpy_case))
    same_report(T.measure_case(hip_case, labels=[2], components=True, min_voxels=5),
                T.measure_case(numpy_case, labels=[2], components=True, min_voxels=5))
    # return_device=True: raw tables, where the volume lives
    raw = T.measure_case(hip_case, labels=[1], return_device=True)['structures'][0]
    assert raw['label'] == 1 and raw['count'] == 1
    assert all(raw[k].is_cuda for k in ('moments', 'faces', 'feret_d2', 'feret_pair'))
    mask = (v == 1).view(np.uint8)
    assert np.array_equal(raw['moments'].cpu().numpy(), M.moments(mask, 1))
    assert np.array_equal(raw['faces'].cpu().numpy(), M.faces(mask, 1, v, 256))
    assert hip_case['pred'].is_cuda


def test_gap_on_the_device_equals_scipy():
    v = case("classes")[0]
    a, b = (v == 1).view(np.uint8), (v == 3).view(np.uint8)
    want = M.gap_mm(a, b, (0.8, 0.8, 3.0))
    assert M.gap_mm(upload(a), upload(b), (0.8, 0.8, 3.0)) == pytest.approx(want, rel=1e-14)
    assert M.gap_mm(upload(a), upload(np.zeros_like(b)), (0.8, 0.8, 3.0)) is None
