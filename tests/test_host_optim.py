"""The host side of optim.SGD / optim.AdamW / optim.Adam(max_grad_norm=): constructor checks, checkpoint interchange with
torch.optim, the scalar rows a captured step uploads, and the Trainer's decision whether a step is captured.  No GPU."""
import types

import pytest
import torch

import optim


def _params():
    return [torch.nn.Parameter(torch.arange(6, dtype=torch.float32).reshape(2, 3)), torch.nn.Parameter(torch.ones(4))]


# ------------------------------------------------------------------------------------------------ constructors
@pytest.mark.parametrize("kw", [dict(lr=-1.0), dict(lr=0.1, momentum=-0.5), dict(lr=0.1, weight_decay=-1e-3),
                                dict(lr=0.1, nesterov=True), dict(lr=0.1, nesterov=True, momentum=0.9, dampening=0.1),
                                dict(lr=0.1, momentum=0.9, dampening=0.5), dict(lr=0.1, max_grad_norm=-1.0),
                                dict(lr=0.1, max_grad_norm=float("nan"))])
def test_sgd_rejects_what_torch_rejects_and_dampening(kw):
    with pytest.raises(ValueError):
        optim.SGD(_params(), **kw)
    if "dampening" not in kw and "max_grad_norm" not in kw:
        with pytest.raises(ValueError):
            torch.optim.SGD(_params(), **kw)


@pytest.mark.parametrize("kw", [dict(lr=-1e-3), dict(eps=-1e-8), dict(betas=(1.0, 0.999)), dict(betas=(0.9, -0.1)),
                                dict(betas=(0.9, 1.0)), dict(weight_decay=-0.1), dict(amsgrad=True),
                                dict(max_grad_norm=-2.0)])
def test_adamw_rejects_what_torch_rejects_and_amsgrad(kw):
    with pytest.raises(ValueError):
        optim.AdamW(_params(), **kw)
    if "amsgrad" not in kw and "max_grad_norm" not in kw:
        with pytest.raises(ValueError):
            torch.optim.AdamW(_params(), **kw)


def test_adam_keeps_rejecting_weight_decay_and_amsgrad():
    with pytest.raises(ValueError):
        optim.Adam(_params(), weight_decay=0.1)
    with pytest.raises(ValueError):
        optim.Adam(_params(), amsgrad=True)
    with pytest.raises(ValueError):
        optim.Adam(_params(), max_grad_norm=-1.0)
    assert optim.Adam(_params()).max_grad_norm is None
    assert optim.Adam(_params(), max_grad_norm=12).max_grad_norm == 12.0


def test_defaults_and_the_common_base():
    sgd = optim.SGD(_params(), 0.01, momentum=0.99, nesterov=True, weight_decay=3e-5, max_grad_norm=12)
    g = sgd.param_groups[0]
    assert (g["lr"], g["momentum"], g["dampening"], g["weight_decay"], g["nesterov"]) == (0.01, 0.99, 0, 3e-5, True)
    adamw = optim.AdamW(_params())
    g = adamw.param_groups[0]
    assert (g["lr"], g["betas"], g["eps"], g["weight_decay"], g["amsgrad"]) == (1e-3, (0.9, 0.999), 1e-8, 1e-2, False)
    for opt in (sgd, adamw, optim.Adam(_params())):
        assert isinstance(opt, optim._Fused) and opt.last_grad_norm is None
    # only plain, unclipped Adam has the update kernel that follows the device-side loss scaler
    assert optim.Adam(_params()).captures_with_scaler()
    assert not optim.Adam(_params(), max_grad_norm=1.0).captures_with_scaler()
    assert not sgd.captures_with_scaler() and not adamw.captures_with_scaler()


# ------------------------------------------------------------------------------------------------ checkpoints
def test_sgd_state_dict_interchanges_with_torch():
    ps = _params()
    ours = optim.SGD(ps, 0.05, momentum=0.9, nesterov=True, weight_decay=1e-4)
    for k, p in enumerate(ps):
        ours.state[p] = {"momentum_buffer": torch.full_like(p, float(k + 1))}
    sd = ours.state_dict()
    assert set(sd["state"][0]) == {"momentum_buffer"}
    pt = _params()
    theirs = torch.optim.SGD(pt, 0.1)
    theirs.load_state_dict(sd)
    g = theirs.param_groups[0]
    assert (g["lr"], g["momentum"], g["nesterov"], g["weight_decay"], g["dampening"]) == (0.05, 0.9, True, 1e-4, 0)
    assert torch.equal(theirs.state[pt[1]]["momentum_buffer"], torch.full((4,), 2.0))
    for p in pt:
        p.grad = torch.ones_like(p)
    theirs.step()                                    # torch runs on what it was given
    # and back
    back = optim.SGD(_params(), 1.0)
    back.load_state_dict(theirs.state_dict())
    g = back.param_groups[0]
    assert (g["lr"], g["momentum"], g["nesterov"]) == (0.05, 0.9, True)
    assert torch.equal(back.state[back.param_groups[0]["params"][0]]["momentum_buffer"],
                       theirs.state[pt[0]]["momentum_buffer"])
    # momentum == 0: no state at all, as in torch
    assert optim.SGD(_params(), 0.1).state_dict()["state"] == {}


def test_adamw_state_dict_interchanges_with_torch():
    ps = _params()
    ours = optim.AdamW(ps, lr=2e-3, betas=(0.8, 0.95), eps=1e-6, weight_decay=0.05)
    for k, p in enumerate(ps):
        ours.state[p] = {"step": torch.tensor(7.0), "exp_avg": torch.full_like(p, 0.5 * (k + 1)),
                         "exp_avg_sq": torch.full_like(p, 0.25)}
    sd = ours.state_dict()
    assert set(sd["state"][1]) == {"step", "exp_avg", "exp_avg_sq"}
    pt = _params()
    theirs = torch.optim.AdamW(pt)
    theirs.load_state_dict(sd)
    g = theirs.param_groups[0]
    assert (g["lr"], tuple(g["betas"]), g["eps"], g["weight_decay"]) == (2e-3, (0.8, 0.95), 1e-6, 0.05)
    for p in pt:
        p.grad = torch.ones_like(p)
    theirs.step()
    assert float(theirs.state[pt[0]]["step"]) == 8.0
    back = optim.AdamW(_params())
    back.load_state_dict(theirs.state_dict())
    p0 = back.param_groups[0]["params"][0]
    assert float(back.state[p0]["step"]) == 8.0 and back.state[p0]["step"].device.type == "cpu"
    assert torch.equal(back.state[p0]["exp_avg"], theirs.state[pt[0]]["exp_avg"])
    assert back.param_groups[0]["weight_decay"] == 0.05


# ------------------------------------------------------------------------------------------------ the block map
def test_block_map_has_one_pair_per_chunk_of_every_tensor():
    c = optim._CHUNK
    assert optim._block_map([1, c, c + 1]) == [0, 0, 1, 0, 2, 0, 2, 1]
    assert optim._block_map([]) == []


# ------------------------------------------------------------------------------------------------ captured rows
def _f32(x):
    return float(torch.tensor(x, dtype=torch.float32))


def test_sgd_replay_row():
    opt = optim.SGD(_params(), 0.01, momentum=0.99, nesterov=True, weight_decay=3e-5)
    with pytest.raises(ValueError):
        opt.begin_capture(torch.zeros(2, 8))
    opt._captured = {"hyper": None, "steps": {0: 0.0}}
    row = torch.full((1, 8), 7.0)
    opt.replay_scalars(row)
    assert row[0].tolist() == [_f32(0.01), _f32(0.99), _f32(3e-5), 1.0, 0.0, 0.0, 1.0, 0.0]
    opt.param_groups[0]["lr"] = 0.004                 # a scheduler between replays
    opt.replay_scalars(row, grad_scale=2.0 ** -16)
    assert float(row[0, 0]) == _f32(0.004) and float(row[0, 6]) == 2.0 ** -16
    opt.sync_captured_steps()                         # nothing to write back: SGD has no step count
    assert opt.state_dict()["state"] == {}
    plain = optim.SGD(_params(), 0.5)
    plain._captured = {"hyper": None, "steps": {0: 0.0}}
    plain.replay_scalars(row)
    assert row[0].tolist() == [0.5, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0]


def test_adamw_replay_row():
    ps = _params()
    opt = optim.AdamW(ps, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
    opt._captured = {"hyper": None, "steps": {0: 3.0}}       # as the capture of step 4 leaves it
    for p in ps:
        opt.state[p] = {"step": torch.tensor(4.0), "exp_avg": torch.zeros_like(p), "exp_avg_sq": torch.zeros_like(p)}
    row = torch.zeros(1, 8)
    opt.replay_scalars(row)
    exp = [1e-3, 0.9, 0.999, 1e-8, 1 - 0.9 ** 4, 1 - 0.999 ** 4, 1.0, 1e-2]     # slot 7: the decay, not sqrt(bc2)
    assert row[0].tolist() == [_f32(v) for v in exp]
    opt.param_groups[0]["lr"] = 5e-4
    opt.replay_scalars(row, grad_scale=0.5)
    assert float(row[0, 0]) == _f32(5e-4) and float(row[0, 6]) == 0.5 and float(row[0, 4]) == _f32(1 - 0.9 ** 5)
    assert float(opt.state_dict()["state"][0]["step"]) == 5.0


def test_adam_row_is_unchanged_by_max_grad_norm():
    rows = []
    for mgn in (None, 12.0):
        opt = optim.Adam(_params(), lr=1e-3, max_grad_norm=mgn)
        opt._captured = {"hyper": None, "steps": {0: 9.0}}
        row = torch.zeros(1, 8)
        opt.replay_scalars(row)
        rows.append(row)
    assert torch.equal(rows[0], rows[1]) and float(rows[0][0, 7]) == _f32(float(rows[0][0, 5]) ** 0.5)


# ------------------------------------------------------------------------------------------------ Trainer._graphed_step
def _trainer(optimizer_of, capture_step, fp16, loss=None):
    import loss as L
    import trainer as T
    model = torch.nn.Conv3d(1, 2, 1)                  # a stub: _graphed_step only looks at optimizer, loss and device
    tr = T.Trainer(model=model, optimizer=optimizer_of(model.parameters()), loss=loss or L.HybirdLoss(),
                   capture_step=capture_step, progress=False)
    tr.device = torch.device("cuda", 0)               # what the decision sees for a model on a HIP device
    tr._scaler = optim.LossScaler() if fp16 else None
    return tr


FUSED = {"sgd": lambda ps: optim.SGD(ps, 0.01, momentum=0.99, nesterov=True, weight_decay=3e-5, max_grad_norm=12),
         "adamw": lambda ps: optim.AdamW(ps),
         "adam_clip": lambda ps: optim.Adam(ps, max_grad_norm=1.0),
         "adam": lambda ps: optim.Adam(ps)}


@pytest.mark.parametrize("name", list(FUSED))
def test_graphed_step_decision_table(name):
    import graph
    make = FUSED[name]
    # bf16 / fp32 storage (no scaler): every fused optimizer is captured, asked for or not
    for capture in (None, True):
        tr = _trainer(make, capture, fp16=False)
        step = tr._graphed_step()
        assert isinstance(step, graph.GraphedTrainStep) and step.optimizer is tr.optimizer
    assert _trainer(make, False, fp16=False)._graphed_step() is None
    # fp16: only plain Adam follows the device-side loss scaler
    if name == "adam":
        for capture in (None, True):
            tr = _trainer(make, capture, fp16=True)
            assert isinstance(tr._graphed_step(), graph.GraphedTrainStep)
        return
    tr = _trainer(make, None, fp16=True)
    assert tr._graphed_step() is None and tr._capture_failed          # the eager loop, and the question is not asked again
    assert tr._graphed_step() is None
    with pytest.raises(TypeError):
        _trainer(make, True, fp16=True)._graphed_step()
    with pytest.raises(TypeError):
        graph.GraphedTrainStep(torch.nn.Conv3d(1, 2, 1), torch.nn.MSELoss(), make(_params()), scaler=optim.LossScaler())


def test_graphed_step_still_refuses_foreign_optimizers():
    import graph
    with pytest.raises(TypeError):
        graph.GraphedTrainStep(torch.nn.Conv3d(1, 2, 1), torch.nn.MSELoss(), torch.optim.SGD(_params(), 0.1))
    tr = _trainer(lambda ps: torch.optim.SGD(ps, 0.1), None, fp16=False)
    assert tr._graphed_step() is None
    with pytest.raises(TypeError):
        _trainer(lambda ps: torch.optim.SGD(ps, 0.1), True, fp16=False)._graphed_step()


def test_loss_scaler_hands_the_inverse_scale_to_every_fused_optimizer(monkeypatch):
    """LossScaler.step(): a fused optimizer gets step(grad_scale=1 / scale) and its gradients are only checked; any other
    optimizer gets them unscaled in place."""
    class Lib:
        def __init__(self):
            self.scales = []

        def ru3d_grad_scale_check(self, tab, bm, nblocks, chunk, scale, found, stream):
            self.scales.append(scale)
            return 0

    for make in FUSED.values():
        opt = make(_params())
        seen = {}
        opt.step = lambda grad_scale=1.0: seen.setdefault("grad_scale", grad_scale)
        sc = optim.LossScaler(init_scale=1024.0)
        sc._scale_t = torch.full((), 1024.0)
        sc._found = torch.zeros(1)
        for p in opt.param_groups[0]["params"]:
            p.grad = torch.ones_like(p)
        lib = Lib()
        tab = types.SimpleNamespace(update=lambda params: None, table=torch.zeros(1), block_map=torch.zeros(1), nblocks=1)
        sc._tables[(id(opt), 0)] = tab
        monkeypatch.setattr(optim.N, "lib", lib)
        monkeypatch.setattr(optim, "stream", lambda: None)
        assert sc.step(opt) is True
        monkeypatch.undo()
        assert lib.scales == [1.0] and seen["grad_scale"] == 1.0 / 1024.0
