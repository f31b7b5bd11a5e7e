"""The fp16 loss scaler's life across graph replays, eager steps of another shape, releases and failed captures, on a
real MI355X.  While a step is captured the scaler lives on the device (`ru3d_amp_state`) and the Adam step number of a
replay is `amp_base + device steps + 1`; the invariant held here is

    amp_base + device steps == number of updates really applied

whatever happens between the replays: a clean or an overflowing eager step (the short last batch of an epoch), two of
them, an overflowing replay, a release and a fresh capture, a capture that raises.  Every scenario runs a
`graph.GraphedTrainStep(..., scaler=...)` against the all-eager `optim.LossScaler` loop on the same batches, as
tests/test_gpu_fp16.py::test_fp16_step_replays_from_a_graph_with_the_scaler_on_the_device does, with that test's bound
on the weights.  A batch overflows deterministically: one inf voxel in its image makes every gradient NaN, which the
overflow check flags at any scale.  Run with `-m gpu`."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no HIP device", allow_module_level=True)

import graph  # noqa: E402
import loss as L  # noqa: E402
import network  # noqa: E402
import optim  # noqa: E402
import trainer as T  # noqa: E402
from oracle import unet_oracle as O  # noqa: E402

DEV = torch.device("cuda:0")
H = torch.float16
USUAL, ODD = (32, 32, 32), (32, 32, 16)
SCALER = dict(init_scale=2.0 ** 8, growth_interval=4)
WEIGHT_TOL = 2e-6            # times max(1, max|w|) of the tensor: the bias corrections' last bit (pow on device / host)


def _setup(criterion=None):
    torch.manual_seed(12)
    model = network.ResUnet3D(2, 8, 1, 2).to(DEV).train()
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout3d):
            m.p = 0.0
    network.set_compute_dtype(model, H)
    return (model, optim.Adam(model.parameters(), lr=1e-3), criterion if criterion is not None else L.HybirdLoss(),
            optim.LossScaler(**SCALER))


def _batches(spec):
    """spec: a string of 'a' (usual shape), 'b' (another shape); upper case = the batch overflows."""
    out = []
    for i, ch in enumerate(spec):
        dims = USUAL if ch in "aA" else ODD
        x = O.synth_image((1, 1) + dims, 40 + i)
        if ch.isupper():
            x[0, 0, 3, 4, 5] = float("inf")
        out.append((x.to(DEV), O.phantom_labels(1, dims, 2).to(DEV)))
    return out


def _eager_step(model, opt, crit, sc, x, y):
    opt.zero_grad()
    sc.scale(crit(model(x), y)).backward()
    return sc.step(opt)


def _eager_run(batches, criterion=None):
    model, opt, crit, sc = _setup(criterion)
    log = [_eager_step(model, opt, crit, sc, x, y) for x, y in batches]
    return model, opt, sc, log


def _steps(model, opt):
    return sorted({float(opt.state[p]["step"]) for p in model.parameters() if p in opt.state and opt.state[p]})


def _assert_same(got, want, what):
    (m_g, o_g, sc_g), (m_e, o_e, sc_e, log) = got, want
    assert sc_g._dev is None, what
    assert (sc_g.loss_scale, sc_g.skipped_steps, sc_g.growth_tracker) == \
        (sc_e.loss_scale, sc_e.skipped_steps, sc_e.growth_tracker), what
    assert sc_e.skipped_steps == log.count(False)
    assert _steps(m_g, o_g) == _steps(m_e, o_e) == [float(log.count(True))], (what, _steps(m_g, o_g), log.count(True))
    worst = 0.0
    for (k, a), (_, b) in zip(m_e.state_dict().items(), m_g.state_dict().items()):
        worst = max(worst, (a - b).abs().max().item() / max(1.0, a.abs().max().item()))
    assert worst <= WEIGHT_TOL, "%s: weights differ from the eager loop's by %.3g (bound %.3g)" % (what, worst, WEIGHT_TOL)


def _graphed_run(batches, after=None):
    model, opt, crit, sc = _setup()
    step = graph.GraphedTrainStep(model, crit, opt, warmup=2, scaler=sc)
    for k, (x, y) in enumerate(batches):
        step(x, y)
        if after is not None:
            after(k, step, opt, sc)
    return model, opt, sc, step


@pytest.mark.parametrize("spec", ["aaaaaaabaaaa", "aaaaaabbaaaa"], ids=["one_clean_eager_step", "two_clean_eager_steps"])
def test_clean_eager_step_of_another_shape_between_replays(spec):
    batches = _batches(spec)
    want = _eager_run(batches)
    model, opt, sc, step = _graphed_run(batches)
    assert step.replays == spec.count("a") - 2 and step.eager_steps == 2 + spec.count("b")
    step.release()
    _assert_same((model, opt, sc), want, spec)


def test_overflowing_eager_step_between_replays_keeps_the_step_count():
    """Ten steps of the usual shape (two eager, eight replays), the short batch overflows and is skipped, four more
    replays.  The scaler's block goes back to the device with its count of steps taken at 0 after every eager step; the
    base it is added to has to move up to the count reached, also when the eager step itself was skipped.  When it did
    not (the base then advanced only with an eager step that was applied), the replays after the skipped batch ran with
    t = 3, 4, 5, 6 instead of 11 .. 14, bias corrections of 0.27 .. 0.47 instead of 0.69 .. 0.77: state['step'] came out
    as 6 instead of 14 and the weights 1.3e-3 away from the eager loop's, 652 times the bound (measured on an MI355X
    before the fix).  An optimizer.state_dict() taken right after the skipped batch must see the true count as well."""
    spec = "aaaaaaaaaaBaaaa"
    batches = _batches(spec)
    want = _eager_run(batches)
    assert want[3] == [True] * 10 + [False] + [True] * 4
    for with_state_dict in (False, True):
        seen = []

        def after(k, step, opt, sc):
            if with_state_dict and spec[k] == "B":
                sd = opt.state_dict()
                seen.append(sorted({float(s["step"]) for s in sd["state"].values()}))
                assert sc.state_dict()["ru3d"]["skipped_steps"] == 1

        model, opt, sc, step = _graphed_run(batches, after)
        assert step.replays == 12 and step.eager_steps == 3
        if with_state_dict:
            assert seen == [[10.0]], seen
        assert opt._captured["amp_base"][0] + int(sc._dev.cpu().view(torch.int32)[5]) == 14
        assert sorted({float(s["step"]) for s in opt.state_dict()["state"].values()}) == [14.0]
        step.release()
        _assert_same((model, opt, sc), want, "%s state_dict=%s" % (spec, with_state_dict))


@pytest.mark.parametrize("spec", ["aaaaaaBbaaaa", "aaaaaabBaaaa", "aaaaaaBBaaaa", "aaaaaAbaaaa", "aaaaaABaaaa", "aaAaaaa"],
                         ids=["skipped_then_applied", "applied_then_skipped", "two_skipped", "overflowing_replay_then_eager",
                              "overflowing_replay_then_skipped_eager", "first_replay_overflows"])
def test_skips_of_either_kind_in_a_row(spec):
    batches = _batches(spec)
    want = _eager_run(batches)
    assert want[3] == [ch.islower() for ch in spec]
    model, opt, sc, step = _graphed_run(batches)
    step.release()
    _assert_same((model, opt, sc), want, spec)


def test_release_then_eager_steps_then_a_fresh_capture():
    spec = "aaaaaaAabaaaaa"
    batches = _batches(spec)
    want = _eager_run(batches)
    model, opt, crit, sc = _setup()
    step = graph.GraphedTrainStep(model, crit, opt, warmup=2, scaler=sc)
    for x, y in batches[:7]:
        step(x, y)
    step.release()
    assert sc._dev is None and opt._captured is None and sc.skipped_steps == 1 and _steps(model, opt) == [6.0]
    for x, y in batches[7:9]:
        assert _eager_step(model, opt, crit, sc, x, y) is True
    step = graph.GraphedTrainStep(model, crit, opt, warmup=1, scaler=sc)
    for x, y in batches[9:]:
        step(x, y)
    assert step.replays == 4 and step.eager_steps == 1
    step.release()
    _assert_same((model, opt, sc), want, spec)


# ------------------------------------------------------------------------------------------------ a capture that raises
class NotCapturable(L.HybirdLoss):
    """A fused loss (Trainer's auto mode captures those only) whose forward raises an ordinary Python error while a
    stream is capturing - before any of its kernels is enqueued - and is HybirdLoss otherwise."""

    def __init__(self):
        super().__init__()
        self.values = []
        self.refused = 0

    def forward(self, input, target):
        if torch.cuda.is_current_stream_capturing():
            self.refused += 1
            raise RuntimeError("NotCapturable: this loss does not run inside a capture")
        v = super().forward(input, target)
        self.values.append(v.detach())
        return v


def test_failed_capture_leaves_optimizer_and_scaler_in_eager_mode():
    spec = "aaaAaab"
    batches = _batches(spec)
    want = _eager_run(batches)
    model, opt, crit, sc = _setup(NotCapturable())
    step = graph.GraphedTrainStep(model, crit, opt, warmup=2, scaler=sc)
    step(*batches[0])
    step(*batches[1])
    with pytest.raises(RuntimeError, match="does not run inside a capture"):
        step(*batches[2])
    assert crit.refused == 1
    assert sc._dev is None and opt._captured is None
    assert step.graph is None and not hasattr(step, "x") and not hasattr(step, "stream")
    assert not any(k[1] for k in opt._plans)                           # no captured launch plan stays behind
    assert _steps(model, opt) == [2.0]
    log = [_eager_step(model, opt, crit, sc, x, y) for x, y in batches[2:]]
    assert log == want[3][2:]
    _assert_same((model, opt, sc), want, "eager steps after a failed capture")
    # and a step with a loss that can be captured takes the same optimizer and scaler from here
    step = graph.GraphedTrainStep(model, L.HybirdLoss(), opt, warmup=1, scaler=sc)
    for x, y in _batches("aaa"):
        step(x, y)
    assert step.replays == 2
    step.release()
    assert _steps(model, opt) == [float(want[3].count(True) + 3)]


class Cases(torch.utils.data.Dataset):
    """In-memory synthetic cases in the reference's sample format (dict with 'image' [C, W, H, D] and 'label')."""

    def __init__(self, n):
        self.items = [{"image": O.synth_image((1, 1) + USUAL, 500 + i)[0], "label": O.phantom_labels(1, USUAL, 2)[0]}
                      for i in range(n)]

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]


def _trainer(criterion, capture_step):
    torch.manual_seed(0)
    model = network.ResUnet3D(2, 8, 1, 2).to(DEV)
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout3d):
            m.p = 0.0
    opt = optim.Adam(model.parameters(), lr=1e-4)
    torch.manual_seed(11)
    np.random.seed(11)
    return T.Trainer(model=model, optimizer=opt, loss=criterion, dataset=Cases(6), batch_size=1, valid_split=0.0,
                     dataloader_kwargs={"num_workers": 0}, progress=False, capture_step=capture_step)


def test_trainer_auto_mode_falls_back_to_the_eager_loop_when_the_fp16_capture_fails():
    crit_e = NotCapturable()
    tr_e = _trainer(crit_e, False)
    best_e = tr_e.fit(num_epochs=1, use_amp=True, opt_level="O1")
    assert crit_e.refused == 0 and len(crit_e.values) == 6
    crit_a = NotCapturable()
    tr_a = _trainer(crit_a, None)
    best_a = tr_a.fit(num_epochs=1, use_amp=True, opt_level="O1")
    assert crit_a.refused == 1 and tr_a._capture_failed and tr_a._graphed is None
    assert tr_a._scaler._dev is None and tr_a.optimizer._captured is None
    assert len(crit_a.values) == 6                                      # the batch whose capture failed was not lost
    assert [float(v) for v in crit_a.values] == [float(v) for v in crit_e.values]
    assert best_a == best_e
    assert tr_a._scaler.state_dict() == tr_e._scaler.state_dict()
    for a, b in zip(tr_a.model.state_dict().values(), tr_e.model.state_dict().values()):
        assert torch.equal(a, b)


def test_trainer_capture_step_true_still_raises_and_the_trainer_stays_usable():
    crit = NotCapturable()
    tr = _trainer(crit, True)
    with pytest.raises(RuntimeError, match="does not run inside a capture"):
        tr.fit(num_epochs=1, use_amp=True, opt_level="O1")
    assert crit.refused == 1
    assert tr._scaler._dev is None and tr.optimizer._captured is None
    tr.loss = L.HybirdLoss()
    tr.graph_stats = None
    best = tr.fit(num_epochs=1, use_amp=True, opt_level="O1")
    assert np.isfinite(best["loss"])
    assert tr.graph_stats["replays"] >= 3 and tr._scaler._dev is None
