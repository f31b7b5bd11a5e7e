"""The optimizer and loss-scaling kernels of csrc/optim.hip, one at a time, against float64 references on a real MI355X:

  ru3d_adam_multi        (through optim.Adam)   vector body / scalar tail, several 16384-element chunks, a row without a
                                                gradient, unaligned tensors, grad_scale, 60 consecutive step numbers
  ru3d_adam_step         (C ABI)                the grid-stride loop
  ru3d_adam_multi_dev    (C ABI)                scalars from the device block optim.Adam.replay_scalars writes
  ru3d_adam_multi_amp    (C ABI)                step number and bias corrections derived on the device
  ru3d_grad_scale_check  (C ABI)                where an inf / nan sits, what is not an overflow, the in-place scaling
  ru3d_amp_update        (C ABI)                apex's schedule with both clamps

Every tensor table lives inside ONE float32 allocation per role (param, grad, exp_avg, exp_avg_sq) with guard words
around and between the tensors, so that a write outside a tensor is seen (Layout, tests/optim_cases.py).

Tolerances of the one-step check (ulp = spacing of float32 at the reference value; the reference is torch.optim.Adam's
formula in float64 on the kernel's own float32 state and on the float32 values of lr / betas / eps / bias corrections
the kernel is handed):
  * exp_avg = b1 m + (1 - b1) g s and exp_avg_sq = b2 v + (1 - b2) (g s)^2 are sums of two float32 terms.  The first term
    carries one rounding, the second up to four (g s, twice in the square, and the two products), the sum one more: the
    error is at most 1 ulp of the result + 2^-22 of the terms' magnitudes.  (1 ulp of the result alone is not a bound: where
    the two terms of exp_avg cancel, the roundings of the terms are many ulps of their small difference.)
  * the parameter: p - (lr / bc1) * m / (sqrt(v) / sqrt(bc2) + eps), evaluated on the kernel's OWN new m and v and on
    the float32 sqrt(bc2) it is handed, has six roundings in the update term (sqrt(v), two divisions, the sum with eps,
    lr / bc1, the product), each at most 2^-24 of the value, i.e. at most one ulp of the update term, and one rounding in
    the difference: 1 ulp of the parameter + 6 ulp of the update term.  (4 ulp would hold for almost every element, but
    it is not a bound.)  A step number off by one moves the update term by 1e-4 .. 0.5 of itself during the first 60
    steps, a few hundred to a million times this tolerance.
Run with `-m gpu`."""
import random

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no HIP device", allow_module_level=True)

import _native as N  # noqa: E402
import optim  # noqa: E402
from optim_cases import (CHUNK, DEV, GUARD, PATTERN, ROLES, SKEWS, Layout, f32,  # noqa: E402
                         make_grads, ulp)

FLT_MAX = 3.4028234663852886e38
DEFAULT_HP = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
OTHER_HP = dict(lr=1e-2, betas=(0.5, 0.9), eps=1e-3)


def moments_ref(g, m, v, b1, b2, gscale):
    """New moments in float64 and the magnitudes of their terms (for the tolerance)."""
    gs = g.double() * gscale
    m1, m2 = b1 * m.double(), (1.0 - b1) * gs
    v1, v2 = b2 * v.double(), (1.0 - b2) * gs * gs
    return m1 + m2, v1 + v2, m1.abs() + m2.abs(), v1 + v2


def assert_one_step(p0, g, m0, v0, p1, m1, v1, t, hp, gscale, what, bc=None):
    """p0 / m0 / v0: float32 state before the step, p1 / m1 / v1: after it, g: the float32 gradients."""
    b1d, b2d = hp["betas"]
    b1, b2, lr, eps, gs = f32(b1d), f32(b2d), f32(hp["lr"]), f32(hp["eps"]), f32(gscale)
    bc1, bc2 = bc if bc is not None else (f32(1.0 - b1d ** t), f32(1.0 - b2d ** t))
    m_ref, v_ref, m_mag, v_mag = moments_ref(g, m0, v0, b1, b2, gs)
    for name, got, ref, mag in (("exp_avg", m1, m_ref, m_mag), ("exp_avg_sq", v1, v_ref, v_mag)):
        err = (got.double() - ref).abs()
        tol = ulp(ref) + 2.0 ** -22 * mag
        bad = err > tol
        assert not bool(bad.any()), "%s step %d: %s off at %d elements, worst %.3g of its bound" % (
            what, t, name, int(bad.sum()), float((err / tol).max()))
    upd = (lr / bc1) * m1.double() / (v1.double().sqrt() / f32(bc2 ** 0.5) + eps)
    p_ref = p0.double() - upd
    err = (p1.double() - p_ref).abs()
    tol = ulp(p_ref) + 6.0 * ulp(upd)
    bad = err > tol
    assert not bool(bad.any()), "%s step %d: parameter off at %d elements, worst %.3g of its bound" % (
        what, t, int(bad.sum()), float((err / tol).max()))


# ------------------------------------------------------------------------------------------------ ru3d_adam_multi
# every layout x every grad_scale at the default hyper-parameters; the other set once per layout and grad_scale
SIXTY = [(skew, gs, DEFAULT_HP) for skew in SKEWS for gs in (1.0, 2.0 ** -16, 1.0 / 3.0)] + \
        [("aligned", 1.0, OTHER_HP), ("unaligned", 1.0 / 3.0, OTHER_HP), ("grad_unaligned", 2.0 ** -16, OTHER_HP)]


@pytest.mark.parametrize("skew,gscale,hp", SIXTY,
                         ids=["%s-s%.3g-%s" % (s, g, "default" if h is DEFAULT_HP else "lr1e-2_b0.5_0.9_eps1e-3")
                              for s, g, h in SIXTY])
def test_adam_multi_sixty_steps(skew, gscale, hp):
    steps = 60
    lay = Layout(SKEWS[skew], seed=5)
    opt, params = lay.adam(**hp)
    before = lay.bits()
    count = sum(lay.sizes[i] for i in lay.live)
    p, m, v = lay.packed("param"), lay.packed("exp_avg"), lay.packed("exp_avg_sq")
    # the all-float64 Adam that starts from the same state
    b1, b2, lr, eps, gs = f32(hp["betas"][0]), f32(hp["betas"][1]), f32(hp["lr"]), f32(hp["eps"]), f32(gscale)
    p64, m64, v64 = p.double(), m.double(), v.double()
    for t in range(1, steps + 1):
        g = make_grads(count, t, 3)
        lay.set_packed("grad", g.to(DEV))
        opt.step(grad_scale=gscale)
        p1, m1, v1 = lay.packed("param"), lay.packed("exp_avg"), lay.packed("exp_avg_sq")
        assert_one_step(p, g, m, v, p1, m1, v1, t, hp, gscale, "adam_multi[%s]" % skew)
        p, m, v = p1, m1, v1
        m64, v64, _, _ = moments_ref(g, m64, v64, b1, b2, gs)
        bc1, bc2 = 1.0 - hp["betas"][0] ** t, 1.0 - hp["betas"][1] ** t
        p64 = p64 - lr / bc1 * m64 / (v64.sqrt() / bc2 ** 0.5 + eps)
    assert all(float(opt.state[params[i]]["step"]) == steps for i in lay.live)
    assert params[lay.null_row] not in opt.state or not opt.state[params[lay.null_row]]
    # trajectory: the only float32 error that accumulates is the rounding of the parameter itself, half an ulp a step
    err = (p.double() - p64).abs().max().item()
    assert err <= steps * 2.0 ** -23 * p64.abs().max().item() + 1e-7, err
    assert torch.isfinite(p).all() and torch.isfinite(m).all() and torch.isfinite(v).all()
    # guards and the four arrays of the row without a gradient: bit-identical; the gradients are never written
    after = lay.assert_outside_untouched(before, "adam_multi[%s]" % skew)
    g_last = lay.packed("grad")
    assert torch.equal(g_last.view(torch.int32), make_grads(count, steps, 3).view(torch.int32))
    assert not torch.equal(after["param"], before["param"])


def test_adam_step_grid_stride_loop():
    """ru3d_adam_step launches at most 4096 workgroups of 256 threads for 1024 elements each: above 4 * 2^20 elements
    every thread goes round its loop more than four times."""
    n = 5 * 2 ** 20 + 3
    gen = torch.Generator().manual_seed(21)
    p0, m0 = torch.randn(n, generator=gen), 0.01 * torch.randn(n, generator=gen)
    v0, g = 1e-4 * torch.rand(n, generator=gen), make_grads(n, 1, 9)
    hp = DEFAULT_HP
    for t, gscale in ((1, 1.0), (7, 1.0 / 3.0)):
        bufs = []
        for src in (p0, g, m0, v0):
            b = torch.full((n + 2 * GUARD,), PATTERN, dtype=torch.int32).view(torch.float32)
            b[GUARD:GUARD + n] = src
            bufs.append(b.to(DEV))
        pd, gd, md, vd = [b[GUARD:GUARD + n] for b in bufs]
        bc1, bc2 = 1.0 - hp["betas"][0] ** t, 1.0 - hp["betas"][1] ** t
        N.note_device(DEV)
        N.check(N.lib.ru3d_adam_step(N.ptr(pd), N.ptr(gd), N.ptr(md), N.ptr(vd), n, hp["lr"], hp["betas"][0],
                                     hp["betas"][1], hp["eps"], bc1, bc2, gscale, N.stream()), "adam_step")
        assert_one_step(p0, g, m0, v0, pd.cpu(), md.cpu(), vd.cpu(), t, hp, gscale, "adam_step")
        assert torch.equal(gd.cpu().view(torch.int32), g.view(torch.int32))
        for b in bufs:
            guards = torch.cat([b[:GUARD], b[GUARD + n:]]).view(torch.int32).cpu()
            assert bool((guards == PATTERN).all())


# ------------------------------------------------------------------------------------------------ the captured forms
def _multi(lay, tab, bm, nblocks, hp, t, gscale):
    b1, b2 = hp["betas"]
    N.note_device(DEV)
    N.check(N.lib.ru3d_adam_multi(N.ptr(tab), N.ptr(bm), nblocks, CHUNK, float(hp["lr"]), float(b1), float(b2),
                                  float(hp["eps"]), 1.0 - b1 ** t, 1.0 - b2 ** t, float(gscale), N.stream()), "adam_multi")


def _hyper_block(opt, t, amp=None, amp_base=None):
    """The [groups, 8] block of one replay, written by optim.Adam.replay_scalars itself."""
    hyper = torch.zeros(1, 8, dtype=torch.float32, device=DEV)
    opt.begin_capture(hyper)
    cap = opt._captured
    cap["steps"][0] = float(t - 1)
    if amp is not None:
        cap["amp"] = amp
        cap["amp_base"][0] = float(amp_base)
    host = torch.zeros(1, 8, dtype=torch.float32)
    opt.replay_scalars(host)
    hyper.copy_(host)
    opt._captured = None
    return hyper, host


@pytest.mark.parametrize("skew", ["aligned", "unaligned"])
def test_adam_multi_dev_reads_the_same_scalars_from_device_memory(skew):
    lay = Layout(SKEWS[skew], seed=6)
    opt, _ = lay.adam(**DEFAULT_HP)
    tab, bm, nblocks = lay.table()
    start = lay.bits()
    for t in (1, 2, 1000):
        lay.restore(start)
        _multi(lay, tab, bm, nblocks, DEFAULT_HP, t, 1.0)
        want = lay.bits()
        lay.restore(start)
        hyper, host = _hyper_block(opt, t)
        assert float(host[0, 6]) == 1.0 and float(host[0, 4]) == f32(1.0 - 0.9 ** t)
        N.note_device(DEV)
        N.check(N.lib.ru3d_adam_multi_dev(N.ptr(tab), N.ptr(bm), nblocks, CHUNK, N.ptr(hyper), N.stream()),
                "adam_multi_dev")
        got = lay.bits()
        for role in ROLES:
            assert torch.equal(got[role], want[role]), (t, role)
        assert not torch.equal(got["param"], start["param"])


def _amp_block(scale, found, tracker=0, skipped=0, steps=0):
    f = torch.zeros(8, dtype=torch.float32)
    i = f.view(torch.int32)
    f[0], f[1], f[2] = scale, 1.0 / scale, found
    i[3], i[4], i[5] = tracker, skipped, steps
    return f.view(torch.uint8).to(DEV)


@pytest.mark.parametrize("steps_dev", [0, 1, 7])
@pytest.mark.parametrize("base", [0, 1, 999, 100000])
def test_adam_multi_amp_derives_the_step_number_on_the_device(base, steps_dev):
    """t = amp_base + device steps + 1, bias corrections from the betas in double (float32 value + residual): the same
    update as ru3d_adam_multi with the host's 1 - beta ** t.  The moments do not depend on the bias corrections and are
    bit-equal.  The bias corrections may differ in their last bit or two (pow on the device, on the host), which moves
    lr / bc1 and sqrt(bc2) by up to 2^-22 + 2^-23 of themselves, and each run then has five roundings of its own on the
    way to the update term: 16 ulp of the update term (1e-6 .. 2e-6 of it) + 2 ulp of the parameter.  Every other tensor
    starts at zero, where the new parameter IS the update term and the parameter's own ulp hides nothing: betas without
    their residuals move the update term by 3.7e-6 of itself at t = 1000, a step number off by one by 2.9e-4."""
    lay = Layout(SKEWS["aligned"], seed=7)
    for k, i in enumerate(lay.live):
        if k % 2 == 0:
            lay.view("param", i).zero_()
    opt, _ = lay.adam(**DEFAULT_HP)
    tab, bm, nblocks = lay.table()
    start = lay.bits()
    scale = 128.0
    t = base + steps_dev + 1
    _multi(lay, tab, bm, nblocks, DEFAULT_HP, t, 1.0 / scale)
    want = {role: lay.packed(role) for role in ROLES}
    want_bits = lay.bits()
    lay.restore(start)
    amp = _amp_block(scale, 0.0, tracker=2, skipped=3, steps=steps_dev)
    hyper, host = _hyper_block(opt, 12345, amp=amp, amp_base=base)       # the host's own count is not what is used
    assert int(host[0, 5:6].view(torch.int32)[0]) == base
    assert abs(float(host[0, 1]) + float(host[0, 4]) - 0.9) < 1e-14 and float(host[0, 4]) != 0.0
    assert abs(float(host[0, 2]) + float(host[0, 7]) - 0.999) < 1e-14 and float(host[0, 7]) != 0.0
    N.note_device(DEV)
    N.check(N.lib.ru3d_adam_multi_amp(N.ptr(tab), N.ptr(bm), nblocks, CHUNK, N.ptr(hyper), N.ptr(amp), N.stream()),
            "adam_multi_amp")
    got_bits = lay.assert_outside_untouched(start, "adam_multi_amp")
    for role in ("grad", "exp_avg", "exp_avg_sq"):
        assert torch.equal(got_bits[role], want_bits[role]), role
    p0 = torch.cat([start["param"][lay.off["param"][i]:lay.off["param"][i] + lay.sizes[i]] for i in lay.live])
    p0 = p0.view(torch.float32).double()
    got, ref = lay.packed("param").double(), want["param"].double()
    err = (got - ref).abs()
    tol = 2.0 * ulp(ref) + 16.0 * ulp(ref - p0)
    assert not bool((err > tol).any()), "base %d steps %d: worst %.3g of the bound" % (base, steps_dev,
                                                                                        float((err / tol).max()))
    assert float((ref - p0).abs().max()) > 0
    assert torch.equal(amp.cpu(), _amp_block(scale, 0.0, tracker=2, skipped=3, steps=steps_dev).cpu())   # read only
    # an overflow was found: the step is skipped, nothing moves
    lay.restore(start)
    amp = _amp_block(scale, 1.0, steps=steps_dev)
    N.check(N.lib.ru3d_adam_multi_amp(N.ptr(tab), N.ptr(bm), nblocks, CHUNK, N.ptr(hyper), N.ptr(amp), N.stream()),
            "adam_multi_amp")
    skipped = lay.bits()
    for role in ROLES:
        assert torch.equal(skipped[role], start[role]), role


# ------------------------------------------------------------------------------------------------ ru3d_grad_scale_check
def _check(tab, bm, nblocks, scale, found):
    N.note_device(DEV)
    N.check(N.lib.ru3d_grad_scale_check(N.ptr(tab), N.ptr(bm), nblocks, CHUNK, float(scale), N.ptr(found), N.stream()),
            "grad_scale_check")
    return float(found.item())


def _placements(lay):
    after_null = lay.null_row + 1
    big = lay.sizes.index(2 * 16384 + 7)
    return [("first element of the table", 0, 0),
            ("last element of a 1-element ragged tail", lay.sizes.index(1025), 1024),
            ("last element of a 3-element ragged tail", lay.sizes.index(1023), 1022),
            ("last element of a chunk", big, CHUNK - 1),
            ("first element of the next chunk", big, CHUNK),
            ("last element of the last chunk's tail", big, 2 * CHUNK + 6),
            ("one element past a whole chunk", lay.sizes.index(16385), 16384),
            ("middle of the largest tensor", lay.sizes.index(100003), 50001),
            ("first element after the row without a gradient", after_null, 0),
            ("last element after the row without a gradient", after_null, lay.sizes[after_null] - 1)]


@pytest.mark.parametrize("skew", ["aligned", "grad_unaligned"])
def test_grad_scale_check_finds_an_overflow_wherever_it_sits(skew):
    lay = Layout(SKEWS[skew], seed=8)
    tab, bm, nblocks = lay.table()
    start = lay.bits()
    found = torch.zeros(1, dtype=torch.float32, device=DEV)
    assert _check(tab, bm, nblocks, 1.0, found) == 0.0
    for what, i, j in _placements(lay):
        for bad in (float("inf"), float("-inf"), float("nan")):
            lay.restore(start)
            lay.view("grad", i)[j] = bad
            found.zero_()
            assert _check(tab, bm, nblocks, 1.0, found) == 1.0, "%s = %s not flagged (%s)" % (what, bad, skew)
            lay.view("grad", i)[j] = 0.0
            found.zero_()
            assert _check(tab, bm, nblocks, 1.0, found) == 0.0, what
    # a flag that is already up stays up after a clean check
    lay.restore(start)
    found.fill_(1.0)
    assert _check(tab, bm, nblocks, 1.0, found) == 1.0
    # the row without a gradient is not read: its (unused) gradient storage may hold anything
    lay.view("grad", lay.null_row).fill_(float("nan"))
    found.zero_()
    assert _check(tab, bm, nblocks, 1.0, found) == 0.0
    assert _check(tab, bm, nblocks, 0.5, found) == 0.0
    assert bool(torch.isnan(lay.view("grad", lay.null_row)).all())


@pytest.mark.parametrize("skew", ["aligned", "grad_unaligned"])
def test_grad_scale_check_does_not_flag_finite_values(skew):
    lay = Layout(SKEWS[skew], seed=9)
    tab, bm, nblocks = lay.table()
    found = torch.zeros(1, dtype=torch.float32, device=DEV)
    for value in (FLT_MAX, -FLT_MAX, 2.0 ** -149, -(2.0 ** -130), 0.0, -0.0):
        for i in lay.live:
            lay.view("grad", i).fill_(value)
        before = lay.bits()
        assert _check(tab, bm, nblocks, 1.0, found) == 0.0, "%r flagged as an overflow" % value
        after = lay.bits()
        for role in ROLES:                      # scale == 1 checks without writing
            assert torch.equal(after[role], before[role]), (value, role)


@pytest.mark.parametrize("scale", [1.0, 2.0 ** -16, 1.0 / 3.0], ids=["s1", "s2^-16", "s1/3"])
@pytest.mark.parametrize("skew", ["aligned", "grad_unaligned"])
def test_grad_scale_check_scales_every_element_in_place(skew, scale):
    lay = Layout(SKEWS[skew], seed=10)
    tab, bm, nblocks = lay.table()
    count = sum(lay.sizes[i] for i in lay.live)
    g = make_grads(count, 1, 4)
    g[5], g[6] = FLT_MAX, -FLT_MAX
    lay.set_packed("grad", g.to(DEV))
    before = lay.bits()
    found = torch.zeros(1, dtype=torch.float32, device=DEV)
    assert _check(tab, bm, nblocks, scale, found) == 0.0
    after = lay.assert_outside_untouched(before, "grad_scale_check")
    for role in ("param", "exp_avg", "exp_avg_sq"):
        assert torch.equal(after[role], before[role]), role
    want = g * torch.tensor(scale, dtype=torch.float32)          # one float32 product per element
    got = lay.packed("grad")
    assert bool((want.abs()[want != 0] >= 2.0 ** -126).all())     # no denormal products: nothing depends on flushing
    bad = got.view(torch.int32) != want.view(torch.int32)
    assert not bool(bad.any()), "%d elements differ from fl32(g * scale), first at %d" % (
        int(bad.sum()), int(bad.nonzero()[0]))


# ------------------------------------------------------------------------------------------------ ru3d_amp_update
class ApexSchedule:
    """apex's dynamic loss scale: halve (not below min) and restart the count on overflow; count a clean step and double
    (not above max) after `interval` of them."""

    def __init__(self, scale, growth, backoff, interval, lo, hi):
        self.scale, self.growth, self.backoff, self.interval, self.lo, self.hi = scale, growth, backoff, interval, lo, hi
        self.tracker = self.skipped = self.steps = 0
        self.at_lo = self.at_hi = 0

    def update(self, found):
        if found:
            self.at_lo += self.scale * self.backoff < self.lo
            self.scale = max(self.scale * self.backoff, self.lo)
            self.tracker = 0
            self.skipped += 1
        else:
            self.steps += 1
            self.tracker += 1
            if self.tracker >= self.interval:
                self.at_hi += self.scale * self.growth > self.hi
                self.scale = min(self.scale * self.growth, self.hi)
                self.tracker = 0


def _amp_fields(amp):
    f = amp.cpu().view(torch.float32)
    i = f.view(torch.int32)
    return dict(scale=float(f[0]), inv_scale=float(f[1]), found_inf=float(f[2]), tracker=int(i[3]), skipped=int(i[4]),
                steps=int(i[5]), reserved=(int(i[6]), int(i[7])))


def test_amp_update_follows_apex_schedule_through_both_clamps():
    kw = (2.0, 0.5, 3, 2.0 ** -3, 2.0 ** 5)
    model = ApexSchedule(1.0, *kw)
    amp = _amp_block(1.0, 0.0)
    found_word = amp[8:12].view(torch.float32)
    rng = random.Random(17)
    N.note_device(DEV)
    events = []
    for k in range(400):
        # stretches that mostly overflow (down to min_scale and against it) and stretches that mostly do not
        p_found = 0.75 if (k // 40) % 2 == 0 else 0.04
        events.append(rng.random() < p_found)
    for k, found in enumerate(events):
        if found:
            found_word.fill_(float("inf") if k % 2 else 1.0)       # any non-zero word is an overflow
        N.check(N.lib.ru3d_amp_update(N.ptr(amp), *kw, N.stream()), "amp_update")
        model.update(found)
        got = _amp_fields(amp)
        want = dict(scale=model.scale, inv_scale=1.0 / model.scale, found_inf=0.0, tracker=model.tracker,
                    skipped=model.skipped, steps=model.steps, reserved=(0, 0))
        assert got == want, (k, found, got, want)
    assert model.at_lo >= 5 and model.at_hi >= 5, (model.at_lo, model.at_hi)      # both clamps were really hit
    assert model.skipped + model.steps == 400


def test_amp_update_rejects_bad_arguments_and_leaves_the_block_alone():
    amp = _amp_block(64.0, 1.0, tracker=2, skipped=5, steps=9)
    before = amp.cpu().clone()
    N.note_device(DEV)
    good = dict(growth=2.0, backoff=0.5, interval=3, lo=2.0 ** -3, hi=2.0 ** 5)
    for change in (dict(growth=0.5), dict(backoff=1.5), dict(backoff=0.0), dict(interval=0), dict(interval=-4),
                   dict(hi=2.0 ** -4), dict(lo=0.0)):
        a = dict(good, **change)
        rc = N.lib.ru3d_amp_update(N.ptr(amp), a["growth"], a["backoff"], a["interval"], a["lo"], a["hi"], N.stream())
        assert rc < 0, change
    assert N.lib.ru3d_amp_update(None, 2.0, 0.5, 3, 2.0 ** -3, 2.0 ** 5, N.stream()) < 0
    torch.cuda.synchronize()
    assert torch.equal(amp.cpu(), before)
    # and the same block with good arguments moves
    N.check(N.lib.ru3d_amp_update(N.ptr(amp), 2.0, 0.5, 3, 2.0 ** -3, 2.0 ** 5, N.stream()), "amp_update")
    assert _amp_fields(amp) == dict(scale=32.0, inv_scale=1.0 / 32.0, found_inf=0.0, tracker=0, skipped=6, steps=9,
                                    reserved=(0, 0))
