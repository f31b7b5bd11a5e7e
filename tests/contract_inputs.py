"""Host volumes of the post-processing cases of tests/test_gpu_scratch_contract.py (morphometry, propagation and hole
filling, keep-largest, the vessel graph, territories, geodesic growth), shared with tests/test_host_contract_inputs.py,
which holds every one of them to what its case is there to exercise.  numpy, scipy and the numpy twins only: no device.

Every builder is made once and returns read-only arrays."""
import functools

import numpy as np
import scipy.ndimage as ndi

import geodesic
import transform as T

VOL = (9, 10, 67)               # three 2048-voxel chunks, the last partial; Z straddles a 64-bit word
SAMPLING = (0.75, 0.5, 3.0)
CUBE = np.ones((3, 3, 3), dtype=bool)
QUANTUM = 2.0 ** -10
FLOOD_TILE = (16, 16, 128)      # PG_TX, PG_TY, PG_TW * 64 of csrc/propagate.hip
FLOOD_FIRST_BATCH = 8           # rounds of the first batch of morphology._flood and of geodesic.grow
FORCED_IDS_CAPACITY = 16        # what skeleton.graph_regrow sets skeleton._ids_capacity to


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


@functools.lru_cache(maxsize=None)
def speckle():
    """the speckle mask of the contract file's _volumes(): the same draw"""
    mask = np.random.RandomState(67).rand(*VOL) < 0.45
    mask[0, 0, 0] = mask[-1, -1, -1] = True
    return _frozen(mask)


# ------------------------------------------------------------------------------------------------ simple paths
def walk(corridor, start, cube=False):
    """the voxels of `corridor` in path order from `start`; asserts that the corridor is one simple path under the face
    (or cube) steps: every voxel has at most two neighbours in it, the start one, and the walk visits all of it"""
    steps = [d for d in np.ndindex(3, 3, 3) if d != (1, 1, 1) and (cube or sum(abs(c - 1) for c in d) == 1)]
    inside = set(map(tuple, np.argwhere(corridor)))

    def neighbours(v):
        return [n for n in (tuple(c + d - 1 for c, d in zip(v, step)) for step in steps) if n in inside]
    assert tuple(start) in inside and len(neighbours(tuple(start))) == 1
    path, before = [tuple(start)], None
    while True:
        around = neighbours(path[-1])
        assert len(around) <= 2, "the corridor branches at %s" % (path[-1],)
        onward = [n for n in around if n != before]
        if not onward:
            break
        before = path[-1]
        path.append(onward[0])
    assert len(path) == len(inside), "the corridor is not one path"
    return path


def tile_of(v, tile):
    return tuple(c // t for c, t in zip(v, tile))


def crossing_rounds(path, tile):
    """a lower bound of the rounds a tiled flood needs along a simple path: a tile runs once per round and reads its
    halo once, at its start, so the crossings a round takes in enter different tiles - the crossings of the path in
    order, cut greedily into runs that enter no tile twice"""
    entered = [tile_of(b, tile) for a, b in zip(path, path[1:]) if tile_of(a, tile) != tile_of(b, tile)]
    rounds, seen = 0, set()
    for t in entered:
        if t in seen:
            rounds, seen = rounds + 1, set()
        seen.add(t)
    return rounds + (1 if seen else 0)


def trip_rounds(path, tile, trips):
    """a lower bound of the rounds geodesic.grow needs along a simple path: a tile makes at most `trips` relaxation trips
    per round, and a trip moves a key by one step; only the steps along y and z inside the busiest tile are counted (a
    thread owns a column along x)"""
    inside = {}
    for a, b in zip(path, path[1:]):
        if tile_of(a, tile) == tile_of(b, tile) and a[0] == b[0]:
            inside[tile_of(a, tile)] = inside.get(tile_of(a, tile), 0) + 1
    return -(-max(inside.values()) // trips)


# ------------------------------------------------------------------------------------------------ floods
FLOOD_SHAPE = (20, 10, 67)      # two tiles of csrc/propagate.hip along x


@functools.lru_cache(maxsize=None)
def flood_zigzag():
    """(seed, allowed, start): a one-voxel corridor in the row y = 1 that crosses the tile boundary between x = 15 and
    x = 16 once in every second z, there and back, and an island of speckle the corridor does not touch; the seed is
    the corridor's first voxel and one voxel of the island that is not allowed (it stays and spreads)"""
    allowed = np.zeros(FLOOD_SHAPE, dtype=bool)
    for i, z in enumerate(range(0, FLOOD_SHAPE[2], 2)):
        allowed[14:18, 1, z] = True
        if z + 1 < FLOOD_SHAPE[2]:
            allowed[17 if i % 2 == 0 else 14, 1, z + 1] = True
    corridor = allowed.copy()
    allowed[2:7, 4:9, :] = np.random.RandomState(20).rand(5, 5, FLOOD_SHAPE[2]) < 0.5
    allowed[4, 6, 30] = False
    allowed[4, 6, 29] = allowed[4, 6, 31] = True
    seed = np.zeros(FLOOD_SHAPE, dtype=bool)
    seed[14, 1, 0] = seed[4, 6, 30] = True
    return _frozen(seed, allowed, corridor) + ((14, 1, 0),)


@functools.lru_cache(maxsize=None)
def flood_cube_seed():
    """the seed of morphology.propagate_cube_border (allowed=None, border_value=1): two voxels of VOL"""
    seed = np.zeros(VOL, dtype=bool)
    seed[4, 5, 33] = seed[0, 9, 66] = True
    return _frozen(seed)


@functools.lru_cache(maxsize=None)
def solid_with_cavities():
    """an ellipsoid in VOL with a tunnel through it along z (open at both ends: not a hole), two enclosed cavities, one
    of them across the word boundary, and a plate that touches a face"""
    x, y, z = np.ogrid[:VOL[0], :VOL[1], :VOL[2]]
    solid = ((x - 4) ** 2 / 14.0 + (y - 4.5) ** 2 / 18.0 + (z - 33) ** 2 / 1600.0 < 1)
    tunnel = (x == 4) & (y == 5)
    solid = solid & ~tunnel
    solid[4, 3, 62:65] = False                  # a cavity across z = 64
    solid[5, 6, 20] = False                     # a one-voxel cavity
    solid = solid | ((x == 7) & (y > 2) & (z > 50))
    return _frozen(solid), _frozen(np.broadcast_to(tunnel, VOL).copy())


# ------------------------------------------------------------------------------------------------ keep-largest
@functools.lru_cache(maxsize=None)
def keep_volume():
    """(mask, labels int32, count, sizes): the speckle mask with two cubes of 27 voxels, the largest components by far
    (a tie among the kept: k = 2 keeps both, and nothing else has their size)"""
    mask = speckle() & (np.random.RandomState(3).rand(*VOL) < 0.5)          # thinned: small components only
    mask = mask.copy()
    for x0, y0, z0 in ((0, 0, 1), (5, 6, 62)):                              # the second across the word boundary
        mask[max(x0 - 1, 0):x0 + 4, max(y0 - 1, 0):y0 + 4, max(z0 - 1, 0):z0 + 4] = False
        mask[x0:x0 + 3, y0:y0 + 3, z0:z0 + 3] = True
    mask[8, 0:4, 40:45] = False
    labels, count = ndi.label(mask)
    sizes = np.bincount(labels.ravel(), minlength=count + 1)[1:]
    return _frozen(mask, labels.astype(np.int32)) + (count, _frozen(sizes))


def keep_largest_numpy(mask, k):
    """the numpy twin of components.keep_largest (tests/postprocess_cases.py): (kept mask, relabelled survivors)"""
    labels, _ = ndi.label(mask)
    sizes = np.bincount(labels.ravel())[1:]
    chosen = np.sort(np.argsort(-sizes, kind='stable')[:k]) + 1
    kept = np.isin(labels, chosen)
    return kept, ndi.label(kept)[0]


# ------------------------------------------------------------------------------------------------ morphometry
@functools.lru_cache(maxsize=None)
def morphometry_ids(id_bytes):
    """(ids, count, other, num_other): id_bytes 4 - the int32 components of the speckle mask, counted two beyond the
    last (ids without a voxel), against the class volume `other`; id_bytes 1 - a uint8 class volume of classes 0 .. 5
    in which class 4 has no voxel and class 5 one, a stray 255 above the count (class mode: other=None)"""
    if id_bytes == 4:
        labels, k = ndi.label(speckle())
        other = (np.indices(VOL).sum(axis=0) % 3).astype(np.uint8)
        return _frozen(labels.astype(np.int32)), k + 2, _frozen(other), 2
    rng = np.random.RandomState(1)
    field = ndi.gaussian_filter(rng.rand(*VOL), 1.5)
    v = np.digitize(field, np.quantile(field, [0.4, 0.65, 0.85])).astype(np.uint8)
    v[4, 5, 30:33] = 255
    v[8, 9, 66] = 5
    return _frozen(v), 5, None, 0


def morphometry_frames(count):
    f = np.random.RandomState(count + 5).normal(size=(count, 3, 4))
    f[:, 0, :] = (1.0, 0.0, 0.0, 0.0)           # an index axis itself: exact
    return f


# ------------------------------------------------------------------------------------------------ the vessel graph
PRUNE_MIN_LENGTH = 12.0


@functools.lru_cache(maxsize=None)
def wire_tree():
    """a wire skeleton in VOL, in the planes x = 4 and x = 5: a trunk along z over the word boundary, a side arm that
    ends in a fork with two short tips (a spur on a spur: pruning takes the tips, then the arm), and a handle that leaves
    the trunk and returns to it (a loop: the stretch of trunk under it is short and hangs on two junctions - no spur)"""
    skel = np.zeros(VOL, dtype=bool)
    skel[4, 1, 0:67] = True                                                 # the trunk
    for k in range(1, 4):
        skel[4, 1 + k, 14 + k] = True                                       # the arm, up to its fork at (4, 4, 17)
    for k in range(1, 4):
        skel[4, 4 + k, 17 + k] = True                                       # one tip goes on diagonally
        skel[4, 4 + k, 17 - k] = True                                       # the other turns back
    skel[5, 2, 59] = skel[5, 2, 67 - 1 - 2] = True                          # the handle: up at z = 58, back at z = 65
    skel[5, 3, 60:64] = True
    return _frozen(skel)


@functools.lru_cache(maxsize=None)
def wire_lumen():
    """the mask the radii of wire_tree are measured in: the wire dilated by the face neighbours"""
    return _frozen(ndi.binary_dilation(wire_tree()))


# ------------------------------------------------------------------------------------------------ territories
@functools.lru_cache(maxsize=None)
def sites():
    """(sites, site_ids, K, region, other): sparse sites in VOL with two that are equally far from the voxels between
    them, ids 1 .. 6, a region that leaves sites outside, a class volume 0 .. 4"""
    rng = np.random.RandomState(4)
    s = rng.rand(*VOL) < 0.02
    s[:, :, 10:15] = False
    s[4, 5, 11] = s[4, 5, 13] = True                                        # (4, 5, 12) is as far from one as from the other
    site_ids = rng.randint(1, 7, int(s.sum())).astype(np.int32)
    region = ndi.binary_dilation(rng.rand(*VOL) < 0.01, iterations=3)
    other = rng.randint(0, 5, VOL).astype(np.uint8)
    return _frozen(s, site_ids) + (6,) + _frozen(region, other)


@functools.lru_cache(maxsize=None)
def site_labels(with_region):
    s, site_ids, _, region, _ = sites()
    index, _ = T._nearest_site_numpy(s, SAMPLING)
    return _frozen(index), _frozen(T._site_assign_numpy(s, site_ids, index, region if with_region else None))


TALLY_BEYOND_LDS = 4000         # K with (K + 1) * 3 cells beyond TR_LDS_CELLS = 8192 of csrc/territory.hip


@functools.lru_cache(maxsize=None)
def organ():
    """(skel, graph of the twin, region, vessel, other): wire_tree inside an organ (its dilation by four, without the
    lumen), the lumen as the vessel, a class volume with a 'tumour'"""
    skel = wire_tree()
    g = T._skeleton_graph_numpy(skel, None, SAMPLING)
    vessel = wire_lumen()
    region = ndi.binary_dilation(skel, iterations=4) & ~vessel
    other = np.zeros(VOL, dtype=np.uint8)
    other[2:6, 3:8, 30:40] = 1
    return skel, g, _frozen(region), vessel, _frozen(other)


# ------------------------------------------------------------------------------------------------ geodesic growth
GEODESIC_TILE = (8, 8, 32)      # _native.GEODESIC_TILE
GEODESIC_TRIPS = 32             # _native.GEODESIC_MAX_TRIPS


def serpentine(shape):
    """(corridor, its voxels in path order): one voxel wide, rows along z at every other y of every other x, joined at
    alternating ends (tests/test_gpu_geodesic.py)"""
    X, Y, Z = shape
    path, up_y, up_z = [], True, True
    for x in range(0, X, 2):
        ys = list(range(0, Y, 2)) if up_y else list(range(0, Y, 2))[::-1]
        for i, y in enumerate(ys):
            zs = list(range(Z)) if up_z else list(range(Z))[::-1]
            path += [(x, y, z) for z in zs]
            up_z = not up_z
            if i + 1 < len(ys):
                path.append((x, (y + ys[i + 1]) // 2, zs[-1]))
        up_y = not up_y
        if x + 2 < X:
            path.append((x + 1, ys[-1], path[-1][2]))
    corridor = np.zeros(shape, dtype=bool)
    corridor[tuple(np.array(path).T)] = True
    assert corridor.sum() == len(path)
    return corridor, path


@functools.lru_cache(maxsize=None)
def grow_masked():
    """(seeds int32, allowed, corridor, start): the speckle mask of VOL with the first tile of csrc/geodesic.hip (and a
    margin of one voxel) cleared and a serpentine corridor carved into it, seeded at its first voxel (label 7); a free
    row along z with the seeds 5 and 4 eight steps apart (the voxel between them is an exact tie: 4 wins); label 2
    twice in the speckle, one of them on a voxel that is not allowed (it stays and spreads)"""
    allowed = speckle().copy()
    allowed[0:8, 0:8, 0:33] = False
    corridor, path = serpentine((7, 7, 32))
    allowed[0:7, 0:7, 0:32] = corridor
    inside = np.zeros(VOL, dtype=bool)
    inside[0:7, 0:7, 0:32] = corridor
    allowed[8, 8:10, 35:62] = False
    allowed[7, 9, 35:62] = False
    allowed[8, 9, 36:61] = True
    seeds = np.zeros(VOL, dtype=np.int32)
    seeds[path[0]] = 7
    seeds[8, 9, 44], seeds[8, 9, 52] = 5, 4
    seeds[2, 3, 60] = seeds[6, 1, 45] = 2
    allowed[2, 3, 60] = False
    allowed[2, 3, 59] = allowed[2, 3, 61] = True
    return _frozen(seeds, allowed, inside) + (path[0],)


@functools.lru_cache(maxsize=None)
def grow_cube():
    """(seeds int32, max_distance): three labels in the open volume, a bound that two steps along z reach"""
    seeds = np.zeros(VOL, dtype=np.int32)
    seeds[1, 2, 5], seeds[7, 8, 40], seeds[4, 4, 64] = 3, 9, 1
    return _frozen(seeds), 6.5


def grow_twin(seeds, allowed, connectivity, max_distance=None):
    weights = geodesic.step_weights(SAMPLING, 3, connectivity, QUANTUM)
    return T._geodesic_numpy(seeds, allowed, weights, geodesic.distance_limit(max_distance, QUANTUM))
