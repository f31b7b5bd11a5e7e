"""The kernels of csrc/optim.hip - gradient norm and clipping coefficient, SGD with (Nesterov) momentum and weight decay,
AdamW, clipped Adam - against float64 references on a real MI355X, then optim.SGD / AdamW / Adam(max_grad_norm=) on a
whole model against torch.optim, captured against eager, through Trainer.fit and through the eager fp16 step.

Layout (tests/optim_cases.py, shared with tests/test_gpu_optim_kernels.py): every tensor table lives inside ONE float32
allocation per role (param, grad, exp_avg, exp_avg_sq) with NaN guard words around and between the tensors and a row
without a gradient in the middle; after every launch the guards and that row are bit-unchanged.

One-step tolerances.  u = 2^-24 (one rounding to nearest moves a value by at most u of itself), ulp(x) = the spacing of
float32 at x (u |x| <= ulp(x)).  The reference is the rule in float64 on the kernel's own float32 state and on the float32
values of the scalars it is handed (gs = grad_scale, c = the clipping coefficient, 1 when there is none).

  SGD:    gh = fl(fl(g gs) c)                 two roundings:                     |gh - g gs c|  <= 2 u |gh|
          d  = fl(gh + fl(wd p))              E_d = ulp(d) + 2 u |gh| + u |wd p|
          b' = fl(fl(mu b) + d)               E_b = ulp(b') + u |mu b| + E_d     NOT ulps of b': where mu b and d cancel,
                                              the roundings of the two terms are many ulps of their small sum
          u_ = b'                             (momentum, no Nesterov) the kernel's own new buffer, nothing to add
          u_ = fl(d + fl(mu b'))              (Nesterov, on the kernel's own b')  E_u = ulp(u_) + u |mu b'| + E_d
          u_ = d                              (mu == 0)                           E_u = E_d
          p' = fl(p - fl(lr u_))              E_p = ulp(p') + ulp(lr u_) + lr E_u
          Each ulp() of a sum holds its one rounding (half an ulp of the computed value, at most one ulp at the reference
          next to it).  4 * 2^-149 is added for products that end among the denormals.
  AdamW:  m' = fl(fl(b1 m) + fl((1 - b1) gh)),  v' = fl(fl(b2 v) + fl(fl((1 - b2) gh) gh)); 1 - beta is exact for
          beta >= 0.5.  First term one rounding; second term of m' three (two in gh, the product), of v' six (gh enters
          twice, two products): |m' - ref| <= ulp(m') + u (|b1 m| + 4 |(1 - b1) gh|),
          |v' - ref| <= ulp(v') + u (b2 v + 7 (1 - b2) gh^2)  - the 4th / 7th share holds the second-order terms.
          p' = fl(fl(p keep) - fl(step * fl(m' / fl(fl(sqrt(v') / fl(sqrt(bc2))) + eps)))), keep = fl(1 - fl(lr wd)),
          step = fl(lr / bc1): keep lies in [0.5, 1] and is off by at most u (its own rounding u / 2, that of lr wd far
          below), the decayed parameter therefore by u |p| + half an ulp, the update term has seven roundings (sqrt(v'),
          sqrt(bc2) - taken on the device in both forms of this kernel -, two divisions, the sum with eps, lr / bc1, the
          product) and the difference one: 3 ulp(p') + 7 ulp(update).
  Norm:   squares and sums in float64 (2^-53 per operation, nothing of it reaches float32), one rounding to float32 after
          grad_scale * sqrt(sum): at most 1 ulp of the float64 numpy value.  coef = fl(max_norm / fl(total + 1e-6)): two
          roundings on the kernel's own total, 2 u of itself.
  clip_grad_norm_: g' = fl(g coef): ulp(g') on the kernel's own coef; against max_norm / (total + 1e-6) in float64 on the
          kernel's own total that is ulp(g') + 2 u |g'|.

Whole model: see the tests.  Run with `-m gpu`."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no HIP device", allow_module_level=True)

import _native as N  # noqa: E402
import _ops as ops  # noqa: E402
import graph  # noqa: E402
import loss as L  # noqa: E402
import network  # noqa: E402
import optim  # noqa: E402
from oracle import unet_oracle as O  # noqa: E402
from optim_cases import (CHUNK, DEV, NULL_SIZE, ROLES, SIZES, SKEWS, Layout, f32,  # noqa: E402
                         make_grads, ulp)

U = 2.0 ** -24
TINY = 4 * 2.0 ** -149


def _worst(err, tol):
    return "%d elements, worst %.3g of its bound" % (int((err > tol).sum()), float((err / tol).max()))


# ------------------------------------------------------------------------------------------------ SGD
def assert_sgd_step(p0, g, b0, p1, b1, hp, gscale, coef, what):
    """float32 state before (p0, b0) and after (p1, b1) one step on the float32 gradients g; the module docstring's bound."""
    lr, mu, wd, gs, c = f32(hp["lr"]), f32(hp.get("momentum", 0)), f32(hp.get("weight_decay", 0)), f32(gscale), f32(coef)
    gh = g.double() * gs * c
    wp = wd * p0.double()
    d = gh + wp
    e_d = ulp(d) + 2 * U * gh.abs() + U * wp.abs() + TINY
    if mu != 0:
        mb = mu * b0.double()
        b_ref = mb + d
        err, tol = (b1.double() - b_ref).abs(), ulp(b_ref) + U * mb.abs() + e_d
        assert not bool((err > tol).any()), "%s: momentum buffer off at %s" % (what, _worst(err, tol))
        if hp.get("nesterov"):
            mb1 = mu * b1.double()
            upd = d + mb1
            e_u = ulp(upd) + U * mb1.abs() + e_d
        else:
            upd, e_u = b1.double(), torch.zeros_like(d)
    else:
        upd, e_u = d, e_d
    p_ref = p0.double() - lr * upd
    err, tol = (p1.double() - p_ref).abs(), ulp(p_ref) + ulp(lr * upd) + lr * e_u + TINY
    assert not bool((err > tol).any()), "%s: parameter off at %s" % (what, _worst(err, tol))


def _sgd_arg(tab, bm, nblocks, hp, gscale, coef=None):
    N.note_device(DEV)
    N.check(N.lib.ru3d_sgd_multi(N.ptr(tab), N.ptr(bm), nblocks, CHUNK, float(hp["lr"]), float(hp.get("momentum", 0)),
                                 float(hp.get("weight_decay", 0)), int(bool(hp.get("nesterov"))), float(gscale),
                                 N.ptr(coef), N.stream()), "sgd_multi")


def _row_of(opt, step_no, gscale):
    """The [1, 8] device block of one replay, written by the optimizer's own replay_scalars."""
    opt._captured = {"hyper": None, "steps": {0: float(step_no - 1)}, "amp": None, "amp_base": {}}
    host = torch.zeros(1, 8, dtype=torch.float32)
    opt.replay_scalars(host, grad_scale=gscale)
    opt._captured = None
    return host.to(DEV)


SGD_CASES = [(mu, nes, wd, gs) for mu in (0.0, 0.9, 0.99) for nes in (False, True) for wd in (0.0, 3e-5)
             for gs in (1.0, 2.0 ** -16) if not (nes and mu == 0.0)]


@pytest.mark.parametrize("skew", list(SKEWS))
@pytest.mark.parametrize("k", range(len(SGD_CASES)),
                         ids=["mu%g-%s-wd%g-s%.3g" % (m, "nesterov" if n else "plain", w, s) for m, n, w, s in SGD_CASES])
def test_sgd_three_steps(k, skew):
    """optim.SGD over the guarded layout, three consecutive steps on make_grads' gradients; after each step the one-step
    bound, and the device-row form (ru3d_sgd_multi_dev on the row replay_scalars writes) gives the same bits.  Every
    case runs under each of the three skews; nesterov with momentum 0 is refused by torch and by the kernel alike."""
    mu, nes, wd, gscale = SGD_CASES[k]
    hp = dict(lr=1e-2, momentum=mu, nesterov=nes, weight_decay=wd)
    lay = Layout(SKEWS[skew], seed=20 + k)
    opt, params = lay.optimizer(optim.SGD, **hp)
    tab, bm, nblocks = lay.table(first=mu != 0, second=False)
    before = lay.bits()
    p, b = lay.packed("param"), lay.packed("exp_avg")
    for t in (1, 2, 3):
        g = make_grads(lay.count, t, 30 + k)
        lay.set_packed("grad", g.to(DEV))
        start = lay.bits()
        opt.step(grad_scale=gscale)
        after = lay.assert_outside_untouched(before, "sgd[%s]" % skew)
        p1, b1 = lay.packed("param"), lay.packed("exp_avg")
        assert_sgd_step(p, g, b, p1, b1, hp, gscale, 1.0, "sgd_multi[%s] step %d" % (skew, t))
        assert torch.equal(after["grad"], start["grad"]) and torch.equal(after["exp_avg_sq"], start["exp_avg_sq"])
        if mu == 0:
            assert torch.equal(after["exp_avg"], start["exp_avg"])
        assert not torch.equal(after["param"], start["param"])
        # the same step from the device row
        lay.restore(start)
        N.note_device(DEV)
        N.check(N.lib.ru3d_sgd_multi_dev(N.ptr(tab), N.ptr(bm), nblocks, CHUNK, N.ptr(_row_of(opt, t, gscale)), None,
                                         N.stream()), "sgd_multi_dev")
        dev = lay.bits()
        for role in ROLES:
            assert torch.equal(dev[role], after[role]), (t, role)
        p, b = p1, b1
    assert torch.isfinite(p).all() and torch.isfinite(b).all()
    if mu == 0:
        assert all(not opt.state[q] for q in params)           # no state without momentum, as in torch


# ------------------------------------------------------------------------------------------------ AdamW
def assert_adamw_step(p0, g, m0, v0, p1, m1, v1, t, hp, gscale, coef, what):
    b1d, b2d = hp["betas"]
    b1, b2, lr, eps, wd = f32(b1d), f32(b2d), f32(hp["lr"]), f32(hp["eps"]), f32(hp["weight_decay"])
    bc1, bc2 = f32(1.0 - b1d ** t), f32(1.0 - b2d ** t)
    gh = g.double() * f32(gscale) * f32(coef)
    ma, mb = b1 * m0.double(), (1.0 - b1) * gh
    va, vb = b2 * v0.double(), (1.0 - b2) * gh * gh
    for name, got, ref, tol in (("exp_avg", m1, ma + mb, ulp(ma + mb) + U * (ma.abs() + 4 * mb.abs()) + TINY),
                                ("exp_avg_sq", v1, va + vb, ulp(va + vb) + U * (va + 7 * vb) + TINY)):
        err = (got.double() - ref).abs()
        assert not bool((err > tol).any()), "%s step %d: %s off at %s" % (what, t, name, _worst(err, tol))
    upd = (lr / bc1) * m1.double() / (v1.double().sqrt() / bc2 ** 0.5 + eps)
    p_ref = p0.double() * (1.0 - lr * wd) - upd
    err, tol = (p1.double() - p_ref).abs(), 3 * ulp(p_ref) + 7 * ulp(upd)
    assert not bool((err > tol).any()), "%s step %d: parameter off at %s" % (what, t, _worst(err, tol))


ADAMW_CASES = [(wd, hp, skew) for wd in (0.0, 1e-2)
               for hp, skew in ((dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8), "aligned"),
                                (dict(lr=1e-2, betas=(0.5, 0.9), eps=1e-3), "unaligned"))] + \
              [(1e-2, dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8), "grad_unaligned")]


@pytest.mark.parametrize("wd,hp,skew", ADAMW_CASES,
                         ids=["wd%g-%s-%s" % (w, "default" if h["eps"] == 1e-8 else "lr1e-2_b0.5_0.9_eps1e-3", s)
                              for w, h, s in ADAMW_CASES])
def test_adamw_ten_steps(wd, hp, skew):
    hp = dict(hp, weight_decay=wd)
    lay = Layout(SKEWS[skew], seed=41)
    opt, params = lay.optimizer(optim.AdamW, **hp)
    tab, bm, nblocks = lay.table()
    before = lay.bits()
    p, m, v = lay.packed("param"), lay.packed("exp_avg"), lay.packed("exp_avg_sq")
    for t in range(1, 11):
        gscale = 1.0 if t % 2 else 2.0 ** -16
        g = make_grads(lay.count, t, 7)
        lay.set_packed("grad", g.to(DEV))
        start = lay.bits()
        opt.step(grad_scale=gscale)
        after = lay.assert_outside_untouched(before, "adamw[%s]" % skew)
        p1, m1, v1 = lay.packed("param"), lay.packed("exp_avg"), lay.packed("exp_avg_sq")
        assert_adamw_step(p, g, m, v, p1, m1, v1, t, hp, gscale, 1.0, "adamw_multi[%s]" % skew)
        assert torch.equal(after["grad"], start["grad"])
        lay.restore(start)
        N.note_device(DEV)
        N.check(N.lib.ru3d_adamw_multi_dev(N.ptr(tab), N.ptr(bm), nblocks, CHUNK, N.ptr(_row_of(opt, t, gscale)), None,
                                           N.stream()), "adamw_multi_dev")
        dev = lay.bits()
        for role in ROLES:
            assert torch.equal(dev[role], after[role]), (t, role)
        p, m, v = p1, m1, v1
    assert all(float(opt.state[params[i]]["step"]) == 10 for i in lay.live)
    assert torch.isfinite(p).all() and torch.isfinite(m).all() and torch.isfinite(v).all()


def test_adamw_without_decay_and_clipped_adam_are_adam_bit_for_bit():
    """weight_decay = 0 multiplies by exactly 1 and a null / unit coefficient changes no bit: what is left is
    ru3d_adam_multi's recurrence.  (AdamW takes sqrtf(bias_corr2) on the device, Adam on the host: both are the correctly
    rounded float32 root, so even that pair agrees; the clipped Adam entry takes the host's, like ru3d_adam_multi.)"""
    hp = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
    lay = Layout(SKEWS["unaligned"], seed=42)
    tab, bm, nblocks = lay.table()
    one = torch.ones(1, dtype=torch.float32, device=DEV)
    start = lay.bits()
    N.note_device(DEV)
    for t in (1, 2, 50):
        bc1, bc2 = 1.0 - 0.9 ** t, 1.0 - 0.999 ** t
        lay.restore(start)
        N.check(N.lib.ru3d_adam_multi(N.ptr(tab), N.ptr(bm), nblocks, CHUNK, 1e-3, 0.9, 0.999, 1e-8, bc1, bc2, 0.25,
                                      N.stream()), "adam_multi")
        want = lay.bits()
        for coef in (None, one):
            lay.restore(start)
            N.check(N.lib.ru3d_adam_multi_clip(N.ptr(tab), N.ptr(bm), nblocks, CHUNK, 1e-3, 0.9, 0.999, 1e-8, bc1, bc2,
                                               0.25, N.ptr(coef), N.stream()), "adam_multi_clip")
            got = lay.bits()
            assert all(torch.equal(got[r], want[r]) for r in ROLES), t
            lay.restore(start)
            opt = optim.Adam([torch.nn.Parameter(torch.zeros(1))], **hp)
            N.check(N.lib.ru3d_adam_multi_clip_dev(N.ptr(tab), N.ptr(bm), nblocks, CHUNK, N.ptr(_row_of(opt, t, 0.25)),
                                                   N.ptr(coef), N.stream()), "adam_multi_clip_dev")
            got = lay.bits()
            assert all(torch.equal(got[r], want[r]) for r in ROLES), t
        lay.restore(start)
        N.check(N.lib.ru3d_adamw_multi(N.ptr(tab), N.ptr(bm), nblocks, CHUNK, 1e-3, 0.9, 0.999, 1e-8, 0.0, bc1, bc2,
                                       0.25, None, N.stream()), "adamw_multi")
        got = lay.bits()
        assert all(torch.equal(got[r], want[r]) for r in ROLES), t


# ------------------------------------------------------------------------------------------------ the norm
def _norm(tab, bm, nblocks, gscale, max_norm, out=None, partials=None):
    partials = torch.full((nblocks,), float("nan"), dtype=torch.float64, device=DEV) if partials is None else partials
    out = torch.full((2,), float("nan"), dtype=torch.float32, device=DEV) if out is None else out
    N.note_device(DEV)
    N.check(N.lib.ru3d_grad_norm(N.ptr(tab), N.ptr(bm), nblocks, CHUNK, N.ptr(partials), float(gscale), float(max_norm),
                                 N.ptr(out), N.stream()), "grad_norm")
    return out, partials


def _norm64(g, gscale=1.0):
    return float(gscale) * float(np.sqrt(np.sum(np.square(g.numpy().astype(np.float64)))))


def _ulps_off(got, ref64):
    r = torch.tensor(ref64, dtype=torch.float64)
    return float(abs(float(got) - ref64) / float(ulp(r)))


@pytest.mark.parametrize("skew", list(SKEWS))
def test_grad_norm_against_float64(skew):
    lay = Layout(SKEWS[skew], seed=50)
    tab, bm, nblocks = lay.table()
    lay.view("grad", lay.null_row).fill_(float("nan"))         # the row without a gradient is not read
    g = 0.1 * torch.randn(lay.count, generator=torch.Generator().manual_seed(51))
    lay.set_packed("grad", g.to(DEV))
    before = lay.bits()
    for gscale, max_norm in ((1.0, 1.0), (2.0 ** -16, 1e-4), (1.0 / 3.0, 1e3)):
        out, partials = _norm(tab, bm, nblocks, gscale, max_norm)
        total, coef = out.cpu().tolist()
        ref = _norm64(g, f32(gscale))
        assert _ulps_off(total, ref) <= 1.0, (skew, gscale, total, ref)
        c_ref = min(1.0, f32(max_norm) / (total + f32(1e-6)))
        assert abs(coef - c_ref) <= 2 * U * c_ref, (coef, c_ref)
        assert (coef == 1.0) == (max_norm == 1e3)
        # a block of the row without a gradient writes 0; the partials are the float64 sums of the chunks
        pc = partials.cpu()
        blocks = bm.cpu().view(-1, 2)
        assert all(float(pc[j]) == 0.0 for j in range(nblocks) if int(blocks[j, 0]) == lay.null_row)
        assert abs(float(pc.sum()) - ref * ref / f32(gscale) ** 2) <= 1e-12 * float(pc.sum())
        # fixed order: a second run gives the same bits, in the partials and in the result
        out2, partials2 = _norm(tab, bm, nblocks, gscale, max_norm)
        assert torch.equal(out2.view(torch.int32), out.view(torch.int32))
        assert torch.equal(partials2.view(torch.int64), partials.view(torch.int64))
    after = lay.bits()
    assert all(torch.equal(after[r], before[r]) for r in ROLES)            # the norm reads only


def test_grad_norm_does_not_depend_on_the_alignment_of_the_gradients():
    outs = []
    g = make_grads(sum(SIZES) - NULL_SIZE, 1, 52)
    for skew in SKEWS:
        lay = Layout(SKEWS[skew], seed=53)
        lay.set_packed("grad", g.to(DEV))
        tab, bm, nblocks = lay.table()
        outs.append(_norm(tab, bm, nblocks, 1.0, 1.0)[1].cpu())
    assert torch.equal(outs[0].view(torch.int64), outs[1].view(torch.int64))
    assert torch.equal(outs[0].view(torch.int64), outs[2].view(torch.int64))


def test_grad_norm_special_values():
    lay = Layout(SKEWS["grad_unaligned"], seed=54)
    tab, bm, nblocks = lay.table()
    # all-zero gradients: norm 0, coefficient 1
    lay.set_packed("grad", torch.zeros(lay.count).to(DEV))
    assert _norm(tab, bm, nblocks, 1.0, 12.0)[0].cpu().tolist() == [0.0, 1.0]
    # 1e18: the float32 squares are inf, the float64 norm is finite
    g = make_grads(lay.count, 1, 55)
    lay.set_packed("grad", g.to(DEV))
    out = _norm(tab, bm, nblocks, 1.0, 12.0)[0].cpu()
    ref = _norm64(g)
    assert 1e19 < ref < 1e21 and _ulps_off(out[0], ref) <= 1.0
    assert abs(float(out[1]) - 12.0 / ref) <= 4 * U * 12.0 / ref
    # a norm below max_norm: exactly 1.0f, also just below (max_norm / (total + 1e-6) rounds to 1 or above)
    small = 0.001 * torch.randn(lay.count, generator=torch.Generator().manual_seed(56))
    lay.set_packed("grad", small.to(DEV))
    total = float(_norm(tab, bm, nblocks, 1.0, 12.0)[0][0])
    for max_norm in (12.0, total * (1 + 1e-5) + 1e-6, total + 2e-6):
        out = _norm(tab, bm, nblocks, 1.0, max_norm)[0].cpu()
        assert float(out[1]) == 1.0 and out[1:].view(torch.int32).item() == 0x3F800000, max_norm
    assert float(_norm(tab, bm, nblocks, 1.0, total * 0.999)[0][1]) < 1.0


@pytest.mark.parametrize("bad", [float("inf"), float("-inf"), float("nan")], ids=["inf", "-inf", "nan"])
def test_clip_with_a_non_finite_gradient_follows_torch(bad):
    """error_if_nonfinite=False: an inf makes the norm inf and the coefficient 0 (finite elements become 0, inf * 0 NaN), a
    NaN makes both NaN and every element NaN - the same set of non-finite elements as torch's function on a CPU copy."""
    torch.manual_seed(57)
    params = [torch.nn.Parameter(torch.zeros(n, device=DEV)) for n in (5, 1025, 16385)]
    cpu = [torch.nn.Parameter(torch.zeros(n)) for n in (5, 1025, 16385)]
    for p, q in zip(params, cpu):
        q.grad = torch.randn(q.numel())
        q.grad[::9] = 0.0
    cpu[1].grad[1024] = bad
    for p, q in zip(params, cpu):
        p.grad = q.grad.to(DEV)
    want = torch.nn.utils.clip_grad_norm_(cpu, 1.0)
    got = optim.clip_grad_norm_(params, 1.0)
    assert got.shape == () and got.device == DEV
    assert torch.equal(torch.isnan(got.cpu()), torch.isnan(want)) and torch.equal(torch.isinf(got.cpu()), torch.isinf(want))
    for p, q in zip(params, cpu):
        assert torch.equal(torch.isfinite(p.grad.cpu()), torch.isfinite(q.grad))
        assert torch.equal(torch.isnan(p.grad.cpu()), torch.isnan(q.grad))
        fin = torch.isfinite(q.grad)
        assert torch.equal(p.grad.cpu()[fin], q.grad[fin])       # zeros (of either sign, compared as values)


# ------------------------------------------------------------------------------------------------ clipping
def _clip_params(lay):
    params = [torch.nn.Parameter(lay.view("param", i)) for i in range(len(lay.sizes))]
    for i in lay.live:
        params[i].grad = lay.view("grad", i)
    return params


@pytest.mark.parametrize("skew", ["aligned", "grad_unaligned"])
def test_clip_grad_norm_scales_in_place(skew):
    lay = Layout(SKEWS[skew], seed=60)
    g = 0.1 * torch.randn(lay.count, generator=torch.Generator().manual_seed(61))
    g[::7] = 0.0
    lay.set_packed("grad", g.to(DEV))
    params = _clip_params(lay)
    before = lay.bits()
    ref = _norm64(g)
    max_norm = ref / 50.0
    total = optim.clip_grad_norm_(params, max_norm)
    assert total.shape == () and total.dtype == torch.float32 and total.device == DEV
    after = lay.assert_outside_untouched(before, "clip_grad_norm_")
    assert all(torch.equal(after[r], before[r]) for r in ("param", "exp_avg", "exp_avg_sq"))
    assert _ulps_off(total, ref) <= 1.0
    coef = f32(max_norm) / (float(total) + f32(1e-6))
    want = g.double() * coef
    err, tol = (lay.packed("grad").double() - want).abs(), ulp(want) + 2 * U * want.abs()
    assert not bool((err > tol).any()), _worst(err, tol)
    assert abs(_norm64(lay.packed("grad")) - max_norm) <= 1e-5 * max_norm
    # a norm below max_norm: the coefficient is exactly 1 and no bit of a gradient moves
    lay.restore(before)
    total = optim.clip_grad_norm_(params, 2.0 * ref)
    assert _ulps_off(total, ref) <= 1.0
    now = lay.bits()
    assert all(torch.equal(now[r], before[r]) for r in ROLES)
    # a single tensor is accepted, as by torch
    lay.restore(before)
    one = optim.clip_grad_norm_(params[-1], 1e-3)
    assert _ulps_off(one, _norm64(g[lay.position(len(SIZES) - 1, 0):])) <= 1.0


FUSED = {"sgd": (optim.SGD, dict(lr=1e-2, momentum=0.99, nesterov=True, weight_decay=3e-5)),
         "adamw": (optim.AdamW, dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)),
         "adam": (optim.Adam, dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8))}


@pytest.mark.parametrize("gscale", [1.0, 2.0 ** -16], ids=["s1", "s2^-16"])
@pytest.mark.parametrize("name", list(FUSED))
def test_fused_clipping(name, gscale):
    """max_grad_norm well below the norm: the step is the rule on g * gscale * coef with the kernel's own coefficient, the
    coefficient is max_norm / (norm + 1e-6) and the norm is that of the gradients times gscale - with 2^-16 the norm of
    the unscaled gradients of an fp16 step.  Then max_grad_norm above the norm: bit-equal to the unclipped optimizer."""
    cls, hp = FUSED[name]
    lay = Layout(SKEWS["unaligned"], seed=62)
    g = (0.1 / gscale) * torch.randn(lay.count, generator=torch.Generator().manual_seed(63))
    g[::5] = 0.0
    lay.set_packed("grad", g.to(DEV))
    ref = _norm64(g, gscale)
    start = lay.bits()
    opt, _ = lay.optimizer(cls, max_grad_norm=ref / 20.0, **hp)
    p, m, v = lay.packed("param"), lay.packed("exp_avg"), lay.packed("exp_avg_sq")
    opt.step(grad_scale=gscale)
    lay.assert_outside_untouched(start, "clipped " + name)
    total = opt.last_grad_norm
    assert total.shape == () and total.device == DEV and _ulps_off(total, ref) <= 1.0
    coef = float(opt._clip[False]["norm"][1])
    c_ref = f32(ref / 20.0) / (float(total) + f32(1e-6))
    assert abs(coef - c_ref) <= 2 * U * c_ref and 0.04 < coef < 0.06
    p1, m1, v1 = lay.packed("param"), lay.packed("exp_avg"), lay.packed("exp_avg_sq")
    assert torch.equal(lay.packed("grad").view(torch.int32), g.view(torch.int32))      # the gradients are only read
    if name == "sgd":
        assert_sgd_step(p, g, m, p1, m1, hp, gscale, coef, "clipped sgd")
    else:
        assert_adamw_step(p, g, m, v, p1, m1, v1, 1, dict(hp, weight_decay=hp.get("weight_decay", 0.0)), gscale, coef,
                          "clipped " + name)
    # the coefficient matters: the unclipped step differs
    lay.restore(start)
    plain, _ = lay.optimizer(cls, **hp)
    plain.step(grad_scale=gscale)
    unclipped = lay.bits()
    assert plain.last_grad_norm is None and not torch.equal(lay.packed("param"), p1)
    lay.restore(start)
    loose, _ = lay.optimizer(cls, max_grad_norm=2.0 * ref, **hp)
    loose.step(grad_scale=gscale)
    got = lay.bits()
    assert float(loose._clip[False]["norm"][1]) == 1.0
    assert all(torch.equal(got[r], unclipped[r]) for r in ROLES)
    assert _ulps_off(loose.last_grad_norm, ref) <= 1.0


def test_max_grad_norm_spans_all_param_groups():
    """Two groups with different learning rates: one norm over both, as torch's function over model.parameters()."""
    torch.manual_seed(64)
    a = [torch.nn.Parameter(torch.randn(n, device=DEV)) for n in (7, 20000)]
    b = [torch.nn.Parameter(torch.randn(n, device=DEV)) for n in (1025, 3)]
    for p in a + b:
        p.grad = torch.randn_like(p)
    grads = torch.cat([p.grad.cpu() for p in a + b])
    before = [p.detach().clone() for p in a + b]
    opt = optim.SGD([{"params": a, "lr": 0.5}, {"params": b, "lr": 0.25}], lr=1.0, max_grad_norm=1.0)
    opt.step()
    ref = _norm64(grads)
    assert _ulps_off(opt.last_grad_norm, ref) <= 1.0
    coef = float(opt._clip[False]["norm"][1])
    for p, p0, lr in zip(a + b, before, (0.5, 0.5, 0.25, 0.25)):
        want = p0.double() - lr * (p.grad.double() * coef)
        err, tol = (p.detach().double() - want).abs(), ulp(want) + 2 * ulp(lr * p.grad.double() * coef)
        assert not bool((err > tol).any())


# ------------------------------------------------------------------------------------------------ bad arguments
def test_every_new_entry_rejects_bad_arguments_and_writes_nothing():
    lay = Layout(SKEWS["aligned"], seed=70)
    tab, bm, nblocks = lay.table()
    partials = torch.full((nblocks,), 3.0, dtype=torch.float64, device=DEV)
    out = torch.full((2,), 5.0, dtype=torch.float32, device=DEV)
    hyper = torch.tensor([1e-3, 0.9, 0.999, 1e-8, 0.1, 0.001, 1.0, 0.01], device=DEV)
    one = torch.full((1,), 0.5, dtype=torch.float32, device=DEV)
    before = lay.bits()
    T, B, P, O_, H, C, S = N.ptr(tab), N.ptr(bm), N.ptr(partials), N.ptr(out), N.ptr(hyper), N.ptr(one), N.stream(DEV)
    lib = N.lib
    # (table, block map, nblocks, chunk_elems) in every way they can be wrong
    wrong = [(None, B, nblocks, CHUNK), (T, None, nblocks, CHUNK), (T, B, 0, CHUNK), (T, B, -1, CHUNK), (T, B, nblocks, 0),
             (T, B, nblocks, 1000), (T, B, nblocks, CHUNK + 4), (T, B, nblocks, -CHUNK)]
    calls = []
    for w in wrong:
        calls += [("grad_sumsq", lib.ru3d_grad_sumsq(*w, P, S)),
                  ("grad_norm", lib.ru3d_grad_norm(*w, P, 1.0, 1.0, O_, S)),
                  ("grad_scale_dev", lib.ru3d_grad_scale_dev(*w, C, S)),
                  ("sgd_multi", lib.ru3d_sgd_multi(*w, 0.1, 0.9, 0.0, 1, 1.0, None, S)),
                  ("sgd_multi_dev", lib.ru3d_sgd_multi_dev(*w, H, None, S)),
                  ("adamw_multi", lib.ru3d_adamw_multi(*w, 1e-3, 0.9, 0.999, 1e-8, 0.01, 0.1, 0.001, 1.0, None, S)),
                  ("adamw_multi_dev", lib.ru3d_adamw_multi_dev(*w, H, None, S)),
                  ("adam_multi_clip", lib.ru3d_adam_multi_clip(*w, 1e-3, 0.9, 0.999, 1e-8, 0.1, 0.001, 1.0, C, S)),
                  ("adam_multi_clip_dev", lib.ru3d_adam_multi_clip_dev(*w, H, C, S))]
    ok = (T, B, nblocks, CHUNK)
    calls += [("grad_sumsq no partials", lib.ru3d_grad_sumsq(*ok, None, S)),
              ("grad_norm no partials", lib.ru3d_grad_norm(*ok, None, 1.0, 1.0, O_, S)),
              ("grad_norm no out", lib.ru3d_grad_norm(*ok, P, 1.0, 1.0, None, S)),
              ("grad_norm negative max_norm", lib.ru3d_grad_norm(*ok, P, 1.0, -1.0, O_, S)),
              ("grad_norm nan max_norm", lib.ru3d_grad_norm(*ok, P, 1.0, float("nan"), O_, S)),
              ("grad_norm_finish no partials", lib.ru3d_grad_norm_finish(None, nblocks, 1.0, None, 1.0, O_, S)),
              ("grad_norm_finish no out", lib.ru3d_grad_norm_finish(P, nblocks, 1.0, None, 1.0, None, S)),
              ("grad_norm_finish n = 0", lib.ru3d_grad_norm_finish(P, 0, 1.0, None, 1.0, O_, S)),
              ("grad_norm_finish negative max_norm", lib.ru3d_grad_norm_finish(P, nblocks, 1.0, None, -2.0, O_, S)),
              ("grad_scale_dev no coef", lib.ru3d_grad_scale_dev(*ok, None, S)),
              ("sgd negative lr", lib.ru3d_sgd_multi(*ok, -0.1, 0.9, 0.0, 0, 1.0, None, S)),
              ("sgd negative momentum", lib.ru3d_sgd_multi(*ok, 0.1, -0.9, 0.0, 0, 1.0, None, S)),
              ("sgd negative decay", lib.ru3d_sgd_multi(*ok, 0.1, 0.9, -1e-3, 0, 1.0, None, S)),
              ("sgd nesterov without momentum", lib.ru3d_sgd_multi(*ok, 0.1, 0.0, 0.0, 1, 1.0, None, S)),
              ("sgd nesterov = 2", lib.ru3d_sgd_multi(*ok, 0.1, 0.9, 0.0, 2, 1.0, None, S)),
              ("sgd_dev no hyper", lib.ru3d_sgd_multi_dev(*ok, None, None, S)),
              ("adamw negative lr", lib.ru3d_adamw_multi(*ok, -1e-3, 0.9, 0.999, 1e-8, 0.01, 0.1, 0.001, 1.0, None, S)),
              ("adamw negative eps", lib.ru3d_adamw_multi(*ok, 1e-3, 0.9, 0.999, -1e-8, 0.01, 0.1, 0.001, 1.0, None, S)),
              ("adamw negative decay", lib.ru3d_adamw_multi(*ok, 1e-3, 0.9, 0.999, 1e-8, -0.01, 0.1, 0.001, 1.0, None, S)),
              ("adamw bias_corr1 = 0", lib.ru3d_adamw_multi(*ok, 1e-3, 0.9, 0.999, 1e-8, 0.01, 0.0, 0.001, 1.0, None, S)),
              ("adamw bias_corr2 = 0", lib.ru3d_adamw_multi(*ok, 1e-3, 0.9, 0.999, 1e-8, 0.01, 0.1, 0.0, 1.0, None, S)),
              ("adamw_dev no hyper", lib.ru3d_adamw_multi_dev(*ok, None, None, S)),
              ("adam_clip bias_corr1 = 0", lib.ru3d_adam_multi_clip(*ok, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0.001, 1.0, C, S)),
              ("adam_clip_dev no hyper", lib.ru3d_adam_multi_clip_dev(*ok, None, C, S))]
    failed = [name for name, rc in calls if not rc < 0]
    assert not failed, failed
    torch.cuda.synchronize()
    after = lay.bits()
    assert all(torch.equal(after[r], before[r]) for r in ROLES)
    assert bool((partials == 3.0).all()) and bool((out == 5.0).all()) and float(one) == 0.5
    # and the same buffers with good arguments move
    N.note_device(DEV)
    N.check(lib.ru3d_grad_norm(*ok, P, 1.0, 1.0, O_, S), "grad_norm")
    N.check(lib.ru3d_sgd_multi(*ok, 0.1, 0.9, 0.0, 1, 1.0, None, S), "sgd_multi")
    assert not bool((out == 5.0).any()) and not torch.equal(lay.bits()["param"], before["param"])


# ------------------------------------------------------------------------------------------------ whole model
SHAPE = (2, 1, 32, 32, 32)


def _small_model(seed=7):
    torch.manual_seed(seed)
    model = network.ResUnet3D(2, 8, 1, 3).to(DEV)             # float32 storage: the yardstick below is float32 too
    model.eval()                                              # dropout off
    return model


def _xy():
    return O.synth_image(SHAPE, 321).to(DEV), O.phantom_labels(SHAPE[0], SHAPE[2:], 3).to(DEV)


class _OnCpu:
    """The same recipe in float32 on the CPU: the oracle's forward / backward (torch on the CPU) and torch's optimizer there,
    from the same weights on the same batch."""

    def __init__(self, model, make, clip):
        self.w = {k: torch.nn.Parameter(v.detach().cpu().clone()) for k, v in model.state_dict().items()
                  if v.is_floating_point()}
        self.params = list(self.w.values())
        self.opt, self.clip = make(self.params), clip

    def step(self, x, y):
        _, _, grads = O.train_step({k: p.detach() for k, p in self.w.items()}, x, y, 2)
        for k, p in self.w.items():
            p.grad = grads.get(k)
        if self.clip is not None:
            torch.nn.utils.clip_grad_norm_(self.params, self.clip)
        self.opt.step()

    def state_dict(self):
        return {k: p.detach() for k, p in self.w.items()}


class _Torch:
    def __init__(self, model, make, clip):
        self.params = list(model.parameters())
        self.opt, self.clip = make(self.params), clip

    def zero_grad(self):
        self.opt.zero_grad(set_to_none=True)

    def step(self):
        if self.clip is not None:
            self.norm = torch.nn.utils.clip_grad_norm_(self.params, self.clip)
        self.opt.step()


RECIPES = {
    "sgd": (lambda ps: optim.SGD(ps, 1e-2, momentum=0.99, nesterov=True, weight_decay=3e-5, max_grad_norm=12),
            lambda ps: torch.optim.SGD(ps, 1e-2, momentum=0.99, nesterov=True, weight_decay=3e-5), 12.0),
    "adamw": (lambda ps: optim.AdamW(ps, lr=1e-3), lambda ps: torch.optim.AdamW(ps, lr=1e-3), None),
}


@pytest.fixture(scope="module")
def three_steps():
    """Three steps of each recipe, run once: ours and torch's optimizer on the device, each on its own copy of the model,
    and the whole recipe in float32 on the CPU - from the same weights, on the same batch."""
    x, y = _xy()
    xc, yc = x.cpu(), y.cpu()
    out = {}
    for name, (ours, theirs, clip) in RECIPES.items():
        models = [_small_model() for _ in range(2)]
        w0 = {k: v.detach().clone() for k, v in models[0].state_dict().items()}
        drivers = [ours(models[0].parameters()), _Torch(models[1], theirs, clip)]
        cpu = _OnCpu(models[0], theirs, clip)
        first, norms = None, []
        for step in range(3):
            cpu.step(xc, yc)
            for m, d in zip(models, drivers):
                d.zero_grad()
                L.HybirdLoss()(m(x), y).backward()
                d.step()
            if clip is not None:
                norms.append((float(drivers[0].last_grad_norm), float(drivers[1].norm)))
            if step == 0:
                first = [{k: v.detach().clone() for k, v in m.state_dict().items()} for m in models]
        out[name] = dict(models=models, drivers=drivers, w0=w0, first=first, norms=norms, cpu=cpu.state_dict())
    return out


@pytest.mark.parametrize("name", list(RECIPES))
def test_whole_model_first_step_matches_torch(three_steps, name):
    """Identical weights give identical gradients on the first step (up to the last bit of the bias and head gradients, which
    the float32 kernels reduce with atomics: 2^-23 of the update, inside the shares below), so the two builds of the rule
    must agree to rounding there.  With U = p_torch - p0 the update torch applied:
      SGD + clip: torch's norm is a float32 tree sum over ~2^20 elements (up to ~20 roundings, 2^-19.7 of itself), its
        coefficient reciprocal-times-max_norm, ours two roundings; then about eight roundings on each side on the way to
        lr * u: the updates differ by at most 2^-18 |U|, the parameters by that + one ulp (two final roundings of half an
        ulp).  Nesterov at the first step: u = (1 + mu) d, no cancellation.
      AdamW: |U - decay| <= lr at the first step (|m^ / (sqrt(v^) + eps)| <= 1); about ten roundings on each side:
        2^-19 lr; the decayed parameter differs by keep's last bit (float32 here, a double in torch) and its rounding:
        3 ulp of the parameter in all.  And one difference that is not a rounding of the arithmetic: the kernel (AdamRule,
        the one recurrence of Adam and AdamW) forms 1 - beta from the FLOAT32 beta, torch from the double.  A beta
        in [0.5, 1) is rounded by up to 2^-25, which is 2^-25 / (1 - beta) of 1 - beta: v^ is off by that share
        (3.0e-5 at beta2 = 0.999), its root by half of it, m^ by 2^-25 / (1 - beta1) (3.0e-7), while the bias
        corrections come from the double on both sides: lr * (2^-26 / (1 - beta2) + 2^-25 / (1 - beta1)) more."""
    r = three_steps[name]
    checked = 0
    for (k, p0), pa, pb in zip(r["w0"].items(), r["first"][0].values(), r["first"][1].values()):
        if not p0.is_floating_point():
            continue
        p0, pa, pb = p0.double().cpu(), pa.double().cpu(), pb.double().cpu()
        if name == "sgd":
            tol = ulp(pb) + 2.0 ** -18 * (pb - p0).abs()
        else:
            tol = 3 * ulp(pb) + 1e-3 * (2.0 ** -19 + 2.0 ** -26 / (1 - 0.999) + 2.0 ** -25 / (1 - 0.9))
        err = (pa - pb).abs()
        assert not bool((err > tol).any()), "%s: %s" % (k, _worst(err, tol))
        checked += int((pb != p0).sum())
    assert checked > 1000
    if name == "sgd":
        ours, theirs = r["norms"][0]
        print("gradient norm of the first step: %.9g (torch %.9g)" % (ours, theirs))
        assert abs(ours - theirs) <= 2.0 ** -19 * theirs
    # parameters without a gradient are skipped: no state, not moved
    model, opt = r["models"][0], r["drivers"][0]
    none = [(k, p) for k, p in model.named_parameters() if p.grad is None]
    assert none
    for k, p in none:
        assert not opt.state.get(p) and torch.equal(p.detach(), r["w0"][k]), k


@pytest.mark.parametrize("name", list(RECIPES))
def test_whole_model_three_steps_stay_within_the_drift_of_two_torch_builds(three_steps, name):
    """After the first step the runs see different gradients and drift apart as any two builds of one rule do.  The yardstick
    is measured here, on this model: the same three steps of torch's optimizer in float32 on the CPU (the oracle's forward
    and backward) against torch's optimizer in float32 on the device.  Ours may be 1.5 times as far from torch-on-the-
    device as those two are from each other - ours shares the device's gradients on the first step, so it should be nearer.
    Maximum over all parameters after three steps, measured on an MI355X:
      sgd:   ours vs torch on the device 9.1e-07, torch on the CPU vs torch on the device 2.3e-06
      adamw: ours vs torch on the device 1.6e-03, torch on the CPU vs torch on the device 1.7e-03
    (AdamW moves an element whose gradient is rounding noise by up to lr a step in a direction the noise decides: the
    drift of any two builds saturates near 2 * lr per step on such elements, so the maximum says little there and the
    median over all elements is held to the same yardstick:
      sgd:   median ours vs torch 1.1e-08, torch on the CPU vs torch on the device 2.6e-08
      adamw: median ours vs torch 1.4e-05, torch on the CPU vs torch on the device 1.3e-05)"""
    r = three_steps[name]
    sa, sb = [m.state_dict() for m in r["models"]]
    sc = r["cpu"]
    ours = max(float((sa[k] - sb[k]).abs().max()) for k in sc)
    builds = max(float((sc[k] - sb[k].cpu()).abs().max()) for k in sc)
    typical = float(torch.cat([(sa[k] - sb[k]).abs().flatten() for k in sc]).median())
    typical_builds = float(torch.cat([(sc[k] - sb[k].cpu()).abs().flatten() for k in sc]).median())
    wmax = max(float(sb[k].abs().max()) for k in sc)
    print("%s: ours vs torch %.3g (median %.3g), between torch builds %.3g (median %.3g)"
          % (name, ours, typical, builds, typical_builds))
    assert ours <= 1.5 * builds, (ours, builds)
    # the maximum saturates for AdamW; the typical element does not: the median is held to the same yardstick
    assert typical <= 1.5 * typical_builds, (typical, typical_builds)
    sa = {k: sa[k] for k in sc}
    moved = max(float((sb[k].float() - r["w0"][k].float()).abs().max()) for k in sa if sa[k].is_floating_point())
    assert moved > 100 * 2.0 ** -23 * wmax            # three real steps were taken


@pytest.mark.parametrize("name", list(RECIPES))
def test_whole_model_checkpoints_interchange(three_steps, name):
    r = three_steps[name]
    ours, theirs = r["drivers"][0], r["drivers"][1].opt
    sa, sb = ours.state_dict(), theirs.state_dict()
    assert sa["state"].keys() == sb["state"].keys()
    keys = {"momentum_buffer"} if name == "sgd" else {"step", "exp_avg", "exp_avg_sq"}
    for idx in sa["state"]:
        assert set(sa["state"][idx]) == keys
        for key in keys - {"step"}:
            assert sa["state"][idx][key].shape == sb["state"][idx][key].shape
        if name != "sgd":
            assert float(sa["state"][idx]["step"]) == float(sb["state"][idx]["step"]) == 3.0
    make_ours, make_theirs, _ = RECIPES[name]
    model_t, model_o = _small_model(), _small_model()      # fresh models: the shared runs stay as they are
    fresh_t = make_theirs(list(model_t.parameters()))
    fresh_t.load_state_dict(sa)                      # ours -> torch
    fresh_o = make_ours(list(model_o.parameters()))
    fresh_o.load_state_dict(sb)                      # torch -> ours
    x, y = _xy()
    for m, o in ((model_t, fresh_t), (model_o, fresh_o)):
        before = [p.detach().clone() for p in m.parameters()]
        o.zero_grad()
        L.HybirdLoss()(m(x), y).backward()
        o.step()                                     # both run on what they were given
        assert any(not torch.equal(a, p.detach()) for a, p in zip(before, m.parameters()))
        assert all(bool(torch.isfinite(p).all()) for p in m.parameters())


# ------------------------------------------------------------------------------------------------ captured == eager
def _batches(n, shape=SHAPE):
    out = []
    for i in range(n):
        x = O.synth_image(shape, 900 + i).to(DEV)
        y = O.phantom_labels(shape[0], shape[2:], 3).to(DEV)
        out.append((x, y.flip(1) if i % 2 else y))
    return out


CAPTURED = {
    "sgd": lambda ps: optim.SGD(ps, 1e-2, momentum=0.99, nesterov=True, weight_decay=3e-5, max_grad_norm=0.05),
    "adamw": lambda ps: optim.AdamW(ps, lr=1e-3),
    "adam_clip": lambda ps: optim.Adam(ps, lr=1e-3, max_grad_norm=0.05),
}


def _setup32(make):
    """The model and optimizer of tests/test_gpu_graph.py's _setup: 32 features (the MFMA kernels), Dropout3d on, bf16."""
    torch.manual_seed(3)
    model = network.ResUnet3D(2, 32, 1, 3).to(DEV)
    network.set_compute_dtype(model, torch.bfloat16)
    model.train()
    ops._drop_counter[0] = 0
    return model, make(model.parameters()), L.HybirdLoss()


@pytest.mark.parametrize("name", list(CAPTURED))
def test_captured_step_equals_eager_bit_for_bit(name):
    """Six steps with an LR change in between: losses, weights, optimizer state and last_grad_norm of the replayed graph
    are those of the eager loop.  max_grad_norm = 0.05 lies below every norm (asserted), so the coefficient the captured
    update reads from device memory is below 1 on every step."""
    batches = _batches(6)
    lr_at = {3: 4e-3 if name == "sgd" else 5e-4}
    runs = []
    for graphed in (False, True):
        model, opt, crit = _setup32(CAPTURED[name])
        step = graph.GraphedTrainStep(model, crit, opt, warmup=2) if graphed else None
        losses, norms = [], []
        for i, (x, y) in enumerate(batches):
            if i in lr_at:
                opt.param_groups[0]["lr"] = lr_at[i]
            if graphed:
                losses.append(step(x, y).clone())
            else:
                opt.zero_grad(set_to_none=True)
                loss = crit(model(x), y)
                loss.backward()
                opt.step()
                losses.append(loss.detach().clone())
            if opt.max_grad_norm is not None:
                norms.append(opt.last_grad_norm.clone())
        torch.cuda.synchronize()
        if graphed:
            assert step.replays == 4 and step.eager_steps == 2
            sd = opt.state_dict()
            step.release()
            assert opt._captured is None and not [k for k in opt._plans if k[1]] and True not in opt._clip
        else:
            sd = opt.state_dict()
        runs.append((model, sd, [float(v) for v in losses], [float(v) for v in norms]))
    (m_e, sd_e, l_e, n_e), (m_g, sd_g, l_g, n_g) = runs
    print("%s: gradient norms %s" % (name, n_e))
    assert l_g == l_e, (l_g, l_e)
    assert n_g == n_e
    if name != "adamw":
        # every norm is above max_grad_norm = 0.05: the coefficient the captured update reads from device memory is < 1
        assert len(n_e) == 6 and all(np.isfinite(n_e)) and min(n_e) > 0.05, n_e
    bad = [k for (k, a), (_, b) in zip(m_e.state_dict().items(), m_g.state_dict().items()) if not torch.equal(a, b)]
    assert not bad, bad
    assert sd_e["state"].keys() == sd_g["state"].keys()
    for k in sd_e["state"]:
        for key, a in sd_e["state"][k].items():
            b = sd_g["state"][k][key]
            assert (float(a) == float(b) == 6.0) if key == "step" else torch.equal(a, b), (k, key)


def test_last_grad_norm_follows_eager_steps_between_replays():
    """A batch of another shape (an epoch's short last batch) runs eagerly between replays.  After EVERY step, replayed or
    eager, last_grad_norm is that step's norm - the value the all-eager loop has - and the replays after the eager step
    go on reporting their own."""
    batches = _batches(6)
    batches[3] = (batches[3][0][:1].contiguous(), batches[3][1][:1].contiguous())
    runs = []
    for graphed in (False, True):
        model, opt, crit = _setup32(CAPTURED["sgd"])
        step = graph.GraphedTrainStep(model, crit, opt, warmup=2) if graphed else None
        losses, norms = [], []
        for x, y in batches:
            if graphed:
                losses.append(step(x, y).clone())
            else:
                opt.zero_grad(set_to_none=True)
                loss = crit(model(x), y)
                loss.backward()
                opt.step()
                losses.append(loss.detach().clone())
            norms.append(opt.last_grad_norm.clone())
        torch.cuda.synchronize()
        if graphed:
            assert step.replays == 3 and step.eager_steps == 3
            step.release()
            assert float(opt.last_grad_norm) == float(norms[-1])       # the value survives the release
        runs.append((model, [float(v) for v in losses], [float(v) for v in norms]))
    (m_e, l_e, n_e), (m_g, l_g, n_g) = runs
    assert l_g == l_e and n_g == n_e, (n_g, n_e)
    assert len(set(n_e)) == 6 and min(n_e) > 0.05                      # six different norms, the clip bites on each
    for (k, a), (_, b) in zip(m_e.state_dict().items(), m_g.state_dict().items()):
        assert torch.equal(a, b), k


def test_add_param_group_after_a_clipped_step():
    """The partials of the norm are sized from the groups as they are at each step: a group added after a clipped step is
    part of the next step's norm, and of its update."""
    torch.manual_seed(65)
    a = [torch.nn.Parameter(torch.randn(n, device=DEV)) for n in (7, 20000)]
    b = [torch.nn.Parameter(torch.randn(n, device=DEV)) for n in (40000, 3)]
    for p in a + b:
        p.grad = torch.randn_like(p)
    for cls, hp in ((optim.SGD, dict(lr=0.5)), (optim.AdamW, dict(lr=1e-3))):
        opt = cls(a, max_grad_norm=1.0, **hp)
        opt.step()
        assert _ulps_off(opt.last_grad_norm, _norm64(torch.cat([p.grad.cpu() for p in a]))) <= 1.0
        opt.add_param_group({"params": b})
        before = [p.detach().clone() for p in b]
        opt.step()
        assert _ulps_off(opt.last_grad_norm, _norm64(torch.cat([p.grad.cpu() for p in a + b]))) <= 1.0
        assert all(not torch.equal(p0, p.detach()) for p0, p in zip(before, b))
        if cls is optim.AdamW:
            assert [float(opt.state[p]["step"]) for p in a + b] == [2.0, 2.0, 1.0, 1.0]


def test_clip_grad_norm_on_a_second_model_of_other_sizes():
    """Two parameter lists of the same length and other sizes, one after the other (a width sweep in one process): each gets
    its own norm and every element of its gradients is scaled."""
    for sizes in ((5, 1025), (40000, 70001)):
        params = [torch.nn.Parameter(torch.zeros(n, device=DEV)) for n in sizes]
        g = [torch.randn(n, generator=torch.Generator().manual_seed(n)) for n in sizes]
        for p, gi in zip(params, g):
            p.grad = gi.to(DEV)
        ref = _norm64(torch.cat(g))
        total = optim.clip_grad_norm_(params, ref / 10.0)
        assert _ulps_off(total, ref) <= 1.0
        coef = f32(ref / 10.0) / (float(total) + f32(1e-6))
        for p, gi in zip(params, g):
            want = gi.double() * coef
            err, tol = (p.grad.cpu().double() - want).abs(), ulp(want) + 2 * U * want.abs()
            assert not bool((err > tol).any()), (sizes, _worst(err, tol))
        del params


class Cases(torch.utils.data.Dataset):
    def __init__(self, n=5, classes=3):
        self.items = [{"image": O.synth_image((1, 1, 32, 32, 32), 700 + i)[0],
                       "label": O.phantom_labels(1, (32, 32, 32), classes)[0]} for i in range(n)]

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]


def test_trainer_fit_with_sgd_replays_and_equals_the_eager_fit():
    import trainer as T

    def fit(capture):
        model, opt, crit = _setup32(CAPTURED["sgd"])
        sched = torch.optim.lr_scheduler.PolynomialLR(opt, total_iters=3, power=0.9)
        torch.manual_seed(5)
        np.random.seed(5)
        tr = T.Trainer(model=model, optimizer=opt, loss=crit, dataset=Cases(), batch_size=2, valid_split=0.0,
                       dataloader_kwargs={"num_workers": 0}, progress=False, capture_step=capture, scheduler=sched)
        tr.fit(num_epochs=3)
        torch.cuda.synchronize()
        return tr, model

    tr_e, m_e = fit(False)
    assert tr_e._graphed is None
    tr_g, m_g = fit(None)                 # the default: captured because optimizer and loss are this package's own
    assert tr_g._graphed is None and tr_g.graph_stats["replays"] > 0
    assert tr_e.best_result == tr_g.best_result
    for (k, a), (_, b) in zip(m_e.state_dict().items(), m_g.state_dict().items()):
        assert torch.equal(a, b), k
    assert tr_g.optimizer.param_groups[0]["lr"] == tr_e.optimizer.param_groups[0]["lr"] < 1e-2


# ------------------------------------------------------------------------------------------------ fp16
def _fp16_setup(make):
    torch.manual_seed(12)
    model = network.ResUnet3D(2, 8, 1, 2).to(DEV).train()
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout3d):
            m.p = 0.0
    network.set_compute_dtype(model, torch.float16)
    return model, make(model.parameters()), L.HybirdLoss(), optim.LossScaler(init_scale=2.0 ** 8, growth_interval=4)


FP16 = {
    "sgd": lambda ps: optim.SGD(ps, 1e-2, momentum=0.9, nesterov=True, weight_decay=3e-5, max_grad_norm=1.0),
    "adamw": lambda ps: optim.AdamW(ps, lr=1e-3),
    "adam_clip": lambda ps: optim.Adam(ps, lr=1e-3, max_grad_norm=1.0),
}


@pytest.mark.parametrize("name", list(FP16))
def test_eager_fp16_step_trains_and_skips_on_overflow(name):
    model, opt, crit, sc = _fp16_setup(FP16[name])
    x = O.synth_image((1, 1, 32, 32, 32), 40).to(DEV)
    y = O.phantom_labels(1, (32, 32, 32), 2).to(DEV)
    losses = []
    for _ in range(3):
        opt.zero_grad()
        loss = crit(model(x), y)
        sc.scale(loss).backward()
        assert sc.step(opt) is True
        losses.append(float(loss.detach()))
    assert losses[-1] < losses[0] and sc.skipped_steps == 0
    if opt.max_grad_norm is not None:
        # the norm of the TRUE gradients: 1 / scale went into the norm kernel
        opt.zero_grad()
        sc.scale(crit(model(x), y)).backward()
        scaled = torch.cat([p.grad.flatten().cpu() for p in model.parameters() if p.grad is not None])
        inv = f32(1.0 / sc.loss_scale)
        assert sc.step(opt) is True
        assert _ulps_off(opt.last_grad_norm, _norm64(scaled, inv)) <= 1.0
    # a forced overflow: the step is skipped, nothing moves, the scale halves
    before = [p.detach().clone() for p in model.parameters()]
    state = {k: {n: (v.clone() if torch.is_tensor(v) else v) for n, v in st.items()}
             for k, st in opt.state_dict()["state"].items()}
    scale = sc.loss_scale
    opt.zero_grad()
    sc.scale(crit(model(x), y)).backward()
    next(p for p in model.parameters() if p.grad is not None).grad.view(-1)[3] = float("inf")
    assert sc.step(opt) is False
    assert sc.skipped_steps == 1 and sc.loss_scale == scale / 2
    assert all(torch.equal(a, p.detach()) for a, p in zip(before, model.parameters()))
    now = opt.state_dict()["state"]
    for k, st in state.items():
        for n, v in st.items():
            assert torch.equal(v, now[k][n]) if torch.is_tensor(v) else v == now[k][n], (k, n)


def test_fp16_with_sgd_is_not_captured():
    import trainer as T
    model, opt, crit, sc = _fp16_setup(CAPTURED["sgd"])
    with pytest.raises(TypeError):
        graph.GraphedTrainStep(model, crit, opt, scaler=sc)

    def trainer(capture):
        model, opt, crit, _ = _fp16_setup(CAPTURED["sgd"])
        torch.manual_seed(11)
        np.random.seed(11)
        return T.Trainer(model=model, optimizer=opt, loss=crit, dataset=Cases(4, classes=2), batch_size=1,
                         valid_split=0.0, dataloader_kwargs={"num_workers": 0}, progress=False, capture_step=capture)

    tr = trainer(True)
    with pytest.raises(TypeError):
        tr.fit(num_epochs=1, use_amp=True, opt_level="O1")
    tr = trainer(None)
    w0 = [p.detach().clone() for p in tr.model.parameters()]
    best = tr.fit(num_epochs=1, use_amp=True, opt_level="O1")
    assert np.isfinite(best["loss"]) and tr._graphed is None and tr._capture_failed
    assert not getattr(tr, "graph_stats", None) or tr.graph_stats["replays"] == 0
    assert any(not torch.equal(a, p.detach()) for a, p in zip(w0, tr.model.parameters()))
