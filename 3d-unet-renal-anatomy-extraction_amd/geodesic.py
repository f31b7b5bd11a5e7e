"""Geodesic distance and nearest-seed labels inside a mask on the device (csrc/geodesic.hip): what is nearest along a path
that stays inside the anatomy, and how long that path is.

`propagate` says whether a voxel can be reached and `territory.nearest` what is nearest in a straight line; `grow` is the
question between them: a multi-source shortest-path transform on the 6- or 26-neighbour voxel graph of an `allowed`
PackedMask.  Step lengths are integers - `step_weights` rounds the Euclidean length of every step to a multiple of
`quantum` - and the state is one 64-bit key per voxel, dist << 32 | label, so the answer is the unique least fixpoint of
the relaxation rule of include/ru3d.h ("geodesic distance"): the smallest distance and, among the seeds at that distance,
the smallest label, the same bytes in every run.  Its defining twin is transform._geodesic_numpy.  There is no host
fallback in here: `grow` wants HIP tensors (the numpy route lives in transform.py and trainer.py).  `step_weights` is
host code and serves both routes.
"""
import ctypes
import itertools
import math

import numpy as np
import torch

import _native as N
from _native import check, ptr, stream
from distance import _packed, _spacing
from morphology import _connectivity

UNLIMITED = N.GEODESIC_UNLIMITED
UNREACHED = 0xFFFFFFFF
# the 26 steps in the order of the weights: ascending (dx, dy, dz) without the centre
OFFSETS = tuple(d for d in itertools.product((-1, 0, 1), repeat=3) if d != (0, 0, 0))

# rounds of the last grow of this process, the overshoot of the last batch included
last_rounds = 0


def step_weights(sampling, ndim, connectivity, quantum=2.0 ** -10):
    """uint32 [26]: the length of every step of OFFSETS in quanta, w(d) = rint(sqrt(sum (d_i s_i)^2) / quantum) in float64
    (half to even), for a volume of `ndim` axes with scipy's `sampling`.  connectivity 1 keeps the face steps and 3 all
    26; a step that is not taken, or that moves along an axis the volume does not have, is 0.  Every weight must lie in
    1 .. 2**20: a quantum too fine or too coarse for the spacing raises ValueError."""
    if connectivity not in (1, 3):
        raise ValueError("step_weights: connectivity=%r (1 = the face steps, 3 = all 26)" % (connectivity,))
    quantum = float(quantum)
    if not (math.isfinite(quantum) and quantum > 0):
        raise ValueError("step_weights: quantum=%r (finite and > 0)" % (quantum,))
    s = np.array(_spacing(sampling, ndim), dtype=np.float64)
    weights = np.zeros(26, dtype=np.uint32)
    for k, d in enumerate(OFFSETS):
        if any(d[:3 - ndim]) or (connectivity == 1 and sum(abs(c) for c in d) != 1):
            continue
        w = np.rint(np.sqrt(np.sum((np.array(d, dtype=np.float64) * s) ** 2)) / quantum)
        if not 1 <= w <= N.GEODESIC_MAX_WEIGHT:
            raise ValueError("step_weights: the step %s of length %r is %r quanta with quantum=%r (1 .. 2**20: choose a quantum "
                             "between 2**-20 of the longest and the whole of the shortest step)"
                             % (d, float(np.sqrt(np.sum((np.array(d) * s) ** 2))), float(w), quantum))
        weights[k] = int(w)
    return weights


def distance_limit(max_distance, quantum):
    """The limit of the relaxation rule in quanta: floor(max_distance / quantum), UNLIMITED without a max_distance."""
    if max_distance is None:
        return UNLIMITED
    if not (math.isfinite(float(max_distance)) and max_distance >= 0):
        raise ValueError("max_distance=%r (None, or finite and >= 0)" % (max_distance,))
    return int(min(math.floor(float(max_distance) / float(quantum)), UNLIMITED))


def _seed_volume(seeds, what):
    if not torch.is_tensor(seeds) or seeds.dtype != torch.int32 or not 1 <= seeds.dim() <= 3:
        raise ValueError("%s: seeds must be an int32 HIP tensor of 1 to 3 axes" % what)
    N.require_device(seeds, "%s: seeds" % what)
    if seeds.numel() == 0 or seeds.numel() >= 1 << 31:
        raise ValueError("%s: a volume of %d voxels is not supported (1 .. 2**31 - 1)" % (what, seeds.numel()))
    return seeds.contiguous()


def grow(seeds, allowed=None, sampling=None, structure=None, quantum=2.0 ** -10, max_distance=None, skip_idle=True):
    """(dist, labels) of the int32 HIP volume `seeds` (0: no seed, > 0: the seed's label; a negative value raises) grown
    through the PackedMask `allowed` (None: everywhere): dist is a uint32 HIP volume, the length in quanta of the shortest
    path of allowed voxels to a seed (0xFFFFFFFF where none arrives), labels the int32 volume of the label of the seed it
    comes from, the smallest label among equally near seeds (0 where not reached).  A seed outside `allowed` stays and
    spreads into its allowed neighbours.  structure: None (the face steps) or the full cube (all 26), as in
    morphology.propagate; sampling: scipy's.  max_distance (in sampling units) stops the growth: no step beyond
    floor(max_distance / quantum) quanta is taken.  Without one a distance that does not fit 32 bits raises OverflowError.
    Batches of 8, 16, 32, 64, 64, .. rounds with one download of the counters after each; a batch whose last round
    stored nothing has converged.  skip_idle=False runs every tile in every round: the same bytes, more work."""
    global last_rounds
    seeds = _seed_volume(seeds, "grow")
    shape = tuple(seeds.shape)
    X, Y, Z = (1,) * (3 - len(shape)) + shape
    if allowed is not None:
        _packed(allowed, "grow: allowed")
        if allowed.shape != shape or allowed.device != seeds.device:
            raise ValueError("grow: seeds of shape %s on %s, allowed of shape %s on %s"
                             % (shape, seeds.device, allowed.shape, allowed.device))
    weights = step_weights(sampling, len(shape), _connectivity(structure, len(shape), "grow"), quantum)
    limit = distance_limit(max_distance, quantum)
    c_weights = (ctypes.c_uint32 * 26)(*[int(w) for w in weights])
    keys = torch.empty(shape, dtype=torch.int64, device=seeds.device)
    counters = torch.empty(N.GEODESIC_MAX_ROUNDS + 2, dtype=torch.int32, device=seeds.device)    # changed, then the flags
    changed, flags = counters[:N.GEODESIC_MAX_ROUNDS], counters[N.GEODESIC_MAX_ROUNDS:]
    ws = N.workspace(N.lib.ru3d_geodesic_workspace_bytes(X, Y, Z), seeds.device)
    N.note_device(seeds.device)
    check(N.lib.ru3d_geodesic_init(ptr(seeds), ptr(keys), X, Y, Z, ptr(flags), ptr(ws), ws.numel(), stream()), "geodesic_init")

    def run(rounds, first, skip):
        check(N.lib.ru3d_geodesic_rounds(None if allowed is None else ptr(allowed.bits), 0, ptr(keys), X, Y, Z, c_weights,
                                         limit, rounds, 1 if first else 0, 1 if skip else 0, ptr(changed), ptr(flags),
                                         ptr(ws), ws.numel(), stream()), "geodesic_rounds")
        return counters.cpu()

    rounds, total = 8, 0
    while True:
        host = run(rounds, total == 0, skip_idle)
        total += rounds
        if int(host[N.GEODESIC_MAX_ROUNDS]):
            raise ValueError("grow: a negative value among the seeds (0: no seed, > 0: a label)")
        if int(host[rounds - 1]) == 0:
            break
        rounds = min(2 * rounds, N.GEODESIC_MAX_ROUNDS)
    if int(host[N.GEODESIC_MAX_ROUNDS + 1]):                # maybe a passing state: every tile looks at the fixpoint
        flags[1:].zero_()
        host = run(1, True, False)
        total += 1
        if int(host[N.GEODESIC_MAX_ROUNDS + 1]):
            raise OverflowError("grow: a distance beyond %d quanta of %r - choose a larger quantum, or a max_distance"
                                % (UNLIMITED, quantum))
    last_rounds = total
    dist = torch.empty(shape, dtype=torch.uint32, device=seeds.device)
    labels = torch.empty(shape, dtype=torch.int32, device=seeds.device)
    check(N.lib.ru3d_geodesic_split(ptr(keys), ptr(dist), ptr(labels), X, Y, Z, stream()), "geodesic_split")
    return dist, labels


def millimetres(dist, quantum=2.0 ** -10):
    """float64 tensor: dist * quantum, the distance of `grow` in sampling units; inf where not reached."""
    if not torch.is_tensor(dist) or dist.dtype != torch.uint32:
        raise ValueError("millimetres: dist must be the uint32 tensor of grow")
    quanta = dist.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    out = quanta.to(torch.float64) * float(quantum)
    return torch.where(quanta == UNREACHED, torch.full_like(out, float('inf')), out)
