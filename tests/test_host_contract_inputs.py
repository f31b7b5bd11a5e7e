"""The host volumes of the post-processing cases of tests/test_gpu_scratch_contract.py (tests/contract_inputs.py) hold
what their cases are there to exercise: round counts beyond the first batch, the shape of the vessel graph and of its
pruning, empty and one-voxel ids, ties of size and of distance, a bound that cuts, a capacity that has to grow.  numpy,
scipy and the numpy twins only - no device - so that the GPU cases are not vacuous on any machine."""
import numpy as np
import scipy.ndimage as ndi

import geodesic
import morphometry
import transform as T

import contract_inputs as C


# ------------------------------------------------------------------------------------------------ floods
def test_the_propagated_corridor_needs_a_second_batch_of_rounds():
    seed, allowed, corridor, start = C.flood_zigzag()
    path = C.walk(corridor, start)
    assert len({C.tile_of(v, C.FLOOD_TILE) for v in path}) == 2
    assert C.crossing_rounds(path, C.FLOOD_TILE) > C.FLOOD_FIRST_BATCH
    want = ndi.binary_propagation(seed, mask=allowed)
    assert want[corridor].all()                                             # the flood walks the corridor to its end
    island = allowed & ~corridor
    assert seed[4, 6, 30] and not allowed[4, 6, 30] and want[4, 6, 30]      # the seed that is not allowed stays
    assert 1 < (want & island).sum() < island.sum()                         # spreads, and does not take the whole island
    assert not ndi.binary_dilation(corridor, structure=C.CUBE)[island].any()


def test_the_cube_flood_from_the_border_takes_the_open_volume():
    seed = C.flood_cube_seed()
    want = ndi.binary_propagation(seed, structure=C.CUBE, border_value=1)
    assert seed.sum() == 2 and want.all()


def test_the_solid_has_cavities_and_a_tunnel():
    solid, tunnel = C.solid_with_cavities()
    filled = ndi.binary_fill_holes(solid)
    holes = filled & ~solid
    count = ndi.label(holes)[1]
    assert count == 2 and holes[4, 3, 63] and holes[4, 3, 64] and holes[5, 6, 20]    # one of them across the word boundary
    inside = tunnel & ndi.binary_fill_holes(solid | tunnel)
    assert inside.sum() > 40 and not filled[tunnel].any()                   # the tunnel runs through the solid and stays open


# ------------------------------------------------------------------------------------------------ keep-largest
def test_the_two_largest_components_tie():
    mask, labels, count, sizes = C.keep_volume()
    order = np.argsort(-sizes, kind='stable')
    assert count > 8 and sizes[order[0]] == sizes[order[1]] == 27 > sizes[order[2]]
    kept, relabelled = C.keep_largest_numpy(mask, 2)
    assert kept.sum() == 54 and relabelled.max() == 2
    assert kept[5:8, 6:9, 62:65].all()                                      # the second cube lies across z = 64


# ------------------------------------------------------------------------------------------------ morphometry
def test_the_id_volumes_have_an_empty_id_and_a_one_voxel_id():
    for id_bytes in (4, 1):
        ids, count, other, num_other = C.morphometry_ids(id_bytes)
        assert ids.dtype.itemsize == id_bytes and ids.shape == C.VOL
        n = morphometry.moments(ids, count)[:, 0]
        assert len(n) == count and (n == 0).any() and (n == 1).any() and (n > 1).any()
        assert (other is None) == (id_bytes == 1)
    assert (C.morphometry_ids(1)[0] > 5).any()                              # a value above the count is skipped


# ------------------------------------------------------------------------------------------------ the vessel graph
def spurs_of(g, min_length):
    nodes, found = g['node_table'], []
    for b, row in enumerate(g['branch_table']):
        n0, n1 = int(row[3]), int(row[4])
        if n0 < 1 or not g['length'][b] < min_length:
            continue
        tips = [(tip, far) for tip, far in ((n0, n1), (n1, n0))
                if nodes[tip - 1, 0] == 1 and nodes[tip - 1, 1] == 1 and nodes[far - 1, 1] >= 3]
        if len(tips) == 1:
            found.append(b)
    return found


def test_the_wire_tree_has_nodes_branches_a_loop_and_spurs_for_two_rounds():
    skel = C.wire_tree()
    g = T._skeleton_graph_numpy(skel)
    assert g['nodes'] >= 3 and g['branches'] >= 3
    assert g['n'] > C.FORCED_IDS_CAPACITY                                   # graph_regrow has to label twice
    assert (g['node_table'][:, 0] > 1).any()                                # a node of several voxels
    # a loop: more edges than a tree of its nodes has (the handle and the trunk under it)
    open_ = g['branch_table'][:, 3] >= 1
    assert int(open_.sum()) > g['nodes'] - ndi.label(skel, structure=C.CUBE)[1]
    spurs = spurs_of(g, C.PRUNE_MIN_LENGTH)
    short = [b for b in range(g['branches']) if g['length'][b] < C.PRUNE_MIN_LENGTH and open_[b]]
    assert len(spurs) >= 1 and len(short) > len(spurs)                      # short branches that are no spurs
    pruned, rounds = T._skeleton_prune_numpy(skel, C.PRUNE_MIN_LENGTH)
    assert rounds >= 3                                                      # two rounds erase, the last finds nothing
    once, _ = T._skeleton_prune_numpy(skel, C.PRUNE_MIN_LENGTH, max_rounds=1)
    assert pruned.sum() < once.sum() < skel.sum()
    after = T._skeleton_graph_numpy(pruned)
    kept_short = [b for b in range(after['branches'])
                  if after['length'][b] < C.PRUNE_MIN_LENGTH and after['branch_table'][b, 3] >= 1]
    assert kept_short and not spurs_of(after, C.PRUNE_MIN_LENGTH)           # a short branch survives: it is no spur
    assert skel[4, 1, :].all() and pruned[4, 1, :].all()                    # the trunk stays
    lumen = C.wire_lumen()
    assert lumen[skel].all() and not lumen.all()


# ------------------------------------------------------------------------------------------------ territories
def test_two_sites_are_equally_near():
    s, site_ids, K, region, other = C.sites()
    assert len(site_ids) == s.sum() > 50 and site_ids.min() >= 1 and site_ids.max() <= K
    p = np.argwhere(s).astype(np.float64) * C.SAMPLING
    v = np.array([4, 5, 12], dtype=np.float64) * C.SAMPLING
    d = np.sort(((p - v) ** 2).sum(axis=1))
    assert d[0] == d[1] < d[2]                                              # the tie, and nothing nearer
    index, sq = T._nearest_site_numpy(s, C.SAMPLING)
    assert index[4, 5, 12] == np.ravel_multi_index((4, 5, 11), C.VOL) and sq[4, 5, 12] == d[0]    # the smaller index wins
    assert (s & ~region).any() and region.any() and not region.all()
    assert other.max() == 4                                                 # values above num_other = 2: the last column
    _, labels = C.site_labels(True)
    assert (labels[region] > 0).all() and not labels[~region].any()
    assert (C.TALLY_BEYOND_LDS + 1) * 3 > 8192 >= (K + 1) * 3               # the two paths of the tally


def test_the_organ_has_a_region_a_vessel_and_a_tumour():
    skel, g, region, vessel, other = C.organ()
    assert vessel[skel].all() and not (region & vessel).any() and region.sum() > 500
    assert (other[region] == 1).any() and (other[region] == 0).any()
    assert g['branches'] >= 3 and g['nodes'] >= 3


# ------------------------------------------------------------------------------------------------ geodesic growth
def test_the_masked_growth_needs_a_second_batch_and_has_a_tie():
    seeds, allowed, corridor, start = C.grow_masked()
    path = C.walk(corridor, start)
    assert C.GEODESIC_TILE == (8, 8, 32) and len({C.tile_of(v, C.GEODESIC_TILE) for v in path}) == 1
    assert C.trip_rounds(path, C.GEODESIC_TILE, C.GEODESIC_TRIPS) > C.FLOOD_FIRST_BATCH
    assert not (ndi.binary_dilation(corridor, structure=C.CUBE) & allowed & ~corridor).any()     # nothing else touches it
    assert sorted(set(seeds[seeds > 0].tolist())) == [2, 4, 5, 7]
    dist, labels = C.grow_twin(seeds, allowed, 1)
    assert (labels[corridor] == 7).all() and dist[path[-1]] != geodesic.UNREACHED
    # the exact tie: alone, each of the two seeds reaches (8, 9, 48) at the same distance, and the smaller label has it
    alone = [C.grow_twin(np.where(seeds == label, seeds, 0), allowed, 1)[0][8, 9, 48] for label in (4, 5)]
    assert alone[0] == alone[1] == dist[8, 9, 48] == 4 * 3072 and labels[8, 9, 48] == 4
    # a seed that is not allowed stays and spreads
    assert seeds[2, 3, 60] == 2 and not allowed[2, 3, 60] and dist[2, 3, 60] == 0 and labels[2, 3, 59] == 2
    assert (dist[allowed] == geodesic.UNREACHED).any() and (dist[allowed] != geodesic.UNREACHED).sum() > 1000


def test_the_bound_of_the_open_growth_cuts():
    seeds, max_distance = C.grow_cube()
    assert len(set(seeds[seeds > 0].tolist())) == 3
    dist, labels = C.grow_twin(seeds, None, 3, max_distance)
    reached = dist != geodesic.UNREACHED
    assert 100 < reached.sum() < reached.size // 2 and (labels[~reached] == 0).all()
    assert dist[reached].max() <= int(max_distance / C.QUANTUM)
    free, _ = C.grow_twin(seeds, None, 3)
    assert (free != geodesic.UNREACHED).all() and np.array_equal(free[reached], dist[reached])
