"""Fused optimizers for the native path: ONE kernel launch per param group updates every parameter tensor of the model.

`Adam` is a drop-in for `torch.optim.Adam(params, lr=..., betas=..., eps=...)` as the training scripts construct it
(reference nb_train_iia.py:18: Adam(model.parameters(), lr=1e-4); weight_decay / amsgrad / maximize are
not used by the reference and are rejected here).  The update rule and the state_dict layout
(`state[p] = {'step', 'exp_avg', 'exp_avg_sq'}`) are torch.optim.Adam's, so checkpoints interchange.
Parameters whose `.grad` is None are skipped, exactly like torch (the never-used skip_conv weights and the
conv biases in front of InstanceNorm).

`SGD` (momentum, Nesterov, weight decay) and `AdamW` follow torch.optim.SGD / torch.optim.AdamW the same way (all of them in
csrc/optim.hip),
and all three take `max_grad_norm`: the global L2 norm of the gradients of ALL param groups is reduced on the device
in a fixed order (float64, no atomics), torch.nn.utils.clip_grad_norm_'s coefficient stays in device memory, and the
update kernels multiply it in while they read the gradient - a clipped step reads the gradients once more and writes
nothing extra.  `optimizer.last_grad_norm` is that step's norm as a 0-dim device tensor; nothing is read back unless the
caller reads it (it is a view of one persistent block: the next step overwrites it, `.clone()` a value that is kept).  `clip_grad_norm_` is torch's function on its own.  That is the nnU-Net / KiTS19 recipe (the reference
trains on KiTS19, nb_train_KITS19.py): SGD(momentum=0.99, nesterov=True, weight_decay=3e-5, max_grad_norm=12) under
torch.optim.lr_scheduler.PolynomialLR.  In data-parallel training every rank holds the same averaged gradients after
GradSync.finish_step(), so every rank computes the same norm and no collective is added.
"""
import ctypes

import torch

import _native as N
from _native import check, ptr, stream

_CHUNK = 16384   # elements per workgroup (multiple of 1024)


class _AdamTensor(ctypes.Structure):
    _fields_ = [("param", ctypes.c_void_p), ("grad", ctypes.c_void_p), ("exp_avg", ctypes.c_void_p),
                ("exp_avg_sq", ctypes.c_void_p), ("count", ctypes.c_int64)]


def _block_map(numels):
    """The flat [tensor, chunk] pairs of the kernels' block map: one workgroup per _CHUNK elements of every tensor."""
    blocks = []
    for ti, n in enumerate(numels):
        for c in range((n + _CHUNK - 1) // _CHUNK):
            blocks += [ti, c]
    return blocks


class _Table:
    """A ru3d_adam_tensor table as the multi-tensor kernels take it: the pinned host block the rows are written into, its
    device copy `table`, the `block_map` with `nblocks` pairs, and the event of the last host-to-device copy."""

    def __init__(self):
        self.numels = None
        self.host = self.table = self.block_map = None
        self.nblocks = 0
        self.copied = None

    def prepare(self, numels, device):
        """The allocations, for tensors of these sizes: nothing to do while sizes and device stay as they are.  They are
        not allowed while a stream is capturing, so a captured step calls this beforehand."""
        numels = tuple(numels)
        if self.numels == numels and self.table.device == device:
            return
        self.host = torch.empty(len(numels) * ctypes.sizeof(_AdamTensor), dtype=torch.uint8).pin_memory()
        self.table = torch.empty(self.host.numel(), dtype=torch.uint8, device=device)
        blocks = _block_map(numels)
        self.block_map = torch.tensor(blocks, dtype=torch.int32).to(device)
        self.nblocks = len(blocks) // 2
        self.numels = numels

    def fill(self, rows, capturing):
        """rows: one (param, grad, exp_avg, exp_avg_sq, count) of addresses (None: null) per tensor."""
        if self.copied is not None:
            self.copied.synchronize()        # the previous async H2D of the table has left the host buffer
        arr = (_AdamTensor * len(rows)).from_buffer(self.host.numpy())
        for i, row in enumerate(rows):
            arr[i] = _AdamTensor(*row)
        self.table.copy_(self.host, non_blocking=True)
        if capturing:
            # the copy is a node of the graph (the gradients live at fixed addresses of the graph's memory pool): its
            # memcpy node re-reads the pinned block at every replay, and the block stays as it is
            self.copied = None
        else:
            self.copied = torch.cuda.Event()
            self.copied.record()


def _check_max_grad_norm(max_grad_norm):
    if max_grad_norm is None:
        return None
    max_grad_norm = float(max_grad_norm)
    if not max_grad_norm >= 0.0:
        raise ValueError("Invalid max_grad_norm: %r" % (max_grad_norm,))
    return max_grad_norm


class _Fused(torch.optim.Optimizer):
    """What the fused optimizers share: the pinned table + block map of a param group (`_plan`), the step that fills the
    tables, reduces the gradient norm when `max_grad_norm` is set and issues one update launch per group, and the captured
    mode of graph.GraphedTrainStep (`begin_capture` / `replay_scalars` / `sync_captured_steps` / `end_capture`).  A
    subclass supplies its state (`_slots`), its two launches (`_launch`, `_launch_dev`) and its scalar row (`_row`)."""
    _NAME = "optim"
    _COUNTS_STEPS = True        # state[p]['step'] exists and the update depends on it

    def __init__(self, params, defaults, max_grad_norm=None):
        self.max_grad_norm = _check_max_grad_norm(max_grad_norm)
        super().__init__(params, defaults)
        self._plans = {}
        self._clip = {}             # captured? -> {"partials": float64[blocks of all groups], "norm": self._norm}
        self._norm = None           # device float32[2] = {total, coef}: ONE block for eager and captured steps
        self._captured = None       # graph.GraphedTrainStep: {"hyper": device float32[groups, 8], "steps": [..]}
        # 0-dim device tensor: the norm max_grad_norm clipped the last step's gradients at.  It is a VIEW of the one
        # persistent norm block (a captured step cannot hand out a fresh tensor per replay): the next step, eager or
        # replayed, overwrites it - `.clone()` a value that is to be kept (a list of norms for logging)
        self.last_grad_norm = None

    # ---- subclass hooks
    def _slots(self, p, group, capturing):
        """Create (first step) and return the state tensors of p that travel in (exp_avg, exp_avg_sq); None for none."""
        raise NotImplementedError

    def _launch(self, plan, group, step_no, grad_scale, coef):
        raise NotImplementedError

    def _launch_dev(self, plan, hyper_row, coef):
        raise NotImplementedError

    def _row(self, row, group, step_no, grad_scale):
        raise NotImplementedError

    def _check_group(self, group):
        pass

    def captures_with_scaler(self):
        """A captured fp16 step needs the update kernel that takes its decisions from the device-side loss scaler
        (ru3d_adam_multi_amp): plain Adam without clipping only."""
        return False

    def _plan(self, gi, group, captured=False):
        """Static part of the launch: the _Table of a param group (built once per group and set of parameter sizes; a
        captured step keeps its own table - its memcpy node re-reads the pinned block at every replay)."""
        params = group["params"]
        numels = tuple(p.numel() for p in params)
        plan = self._plans.get((gi, captured))
        if plan is None or plan.numels != numels:
            for p in params:
                N.require_device(p, "parameter")
                if p.dtype != torch.float32 or not p.is_contiguous():
                    raise N.Ru3dError("optim.%s: parameters must be contiguous float32" % self._NAME)
            plan = self._plans[(gi, captured)] = _Table()
            plan.prepare(numels, params[0].device)
        return plan

    def _clip_buffers(self, captured=False):
        """Device memory of the norm: one float64 partial per block of every group, and the {total, coef} block, which
        eager and captured steps share (last_grad_norm is a view of it, whichever kind of step ran last).  Sized from the
        plans of all groups as they are NOW: add_param_group or a group that grew gives new partials."""
        plans = [self._plan(gi, group, captured) for gi, group in enumerate(self.param_groups) if group["params"]]
        nblocks = sum(pl.nblocks for pl in plans)
        dev = plans[0].table.device
        if self._norm is None or self._norm.device != dev:
            self._norm = torch.zeros(2, dtype=torch.float32, device=dev)
        bufs = self._clip.get(captured)
        if bufs is None or bufs["partials"].numel() != nblocks or bufs["partials"].device != dev:
            bufs = {"partials": torch.empty(nblocks, dtype=torch.float64, device=dev)}
            self._clip[captured] = bufs
        bufs["norm"] = self._norm
        return bufs

    @torch.no_grad()
    def step(self, closure=None, grad_scale=1.0):
        """grad_scale: factor applied to every gradient inside the update kernel (1 / loss_scale in fp16 mode)."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        capturing = self._captured is not None and torch.cuda.is_current_stream_capturing()
        if self._captured is not None and not capturing:
            self.sync_captured_steps()           # an eager step between replays continues their step count
        clip = self.max_grad_norm is not None
        bufs = self._clip_buffers(capturing) if clip and any(g["params"] for g in self.param_groups) else None
        ready = []                               # (gi, group, plan, step_no): the groups that have a gradient
        npartials = 0
        for gi, group in enumerate(self.param_groups):
            params = group["params"]
            if not params:
                continue
            self._check_group(group)
            plan = self._plan(gi, group, capturing)
            N.note_device(params[0].device)
            rows = []
            step_no = None
            any_grad = False
            for p in params:
                if p.grad is None:
                    rows.append((p.data_ptr(), None, None, None, p.numel()))
                    continue
                g = p.grad
                if g.dtype != torch.float32 or not g.is_contiguous():
                    g = g.float().contiguous()
                    p.grad = g
                first, second = self._slots(p, group, capturing)
                if self._COUNTS_STEPS:
                    st = self.state[p]
                    st["step"] += 1
                    step_no = float(st["step"]) if step_no is None else step_no
                    if float(st["step"]) != step_no:
                        raise N.Ru3dError("optim.%s: parameters of one group must share the step count" % self._NAME)
                rows.append((p.data_ptr(), g.data_ptr(), None if first is None else first.data_ptr(),
                             None if second is None else second.data_ptr(), p.numel()))
                any_grad = True
            if not any_grad:
                continue
            step_no = 0.0 if step_no is None else step_no
            plan.fill(rows, capturing)
            if clip:
                check(N.lib.ru3d_grad_sumsq(ptr(plan.table), ptr(plan.block_map), plan.nblocks, _CHUNK,
                                            ptr(bufs["partials"][npartials:]), stream()), "grad_sumsq")
                npartials += plan.nblocks
            ready.append((gi, group, plan, step_no))
        coef = None
        if clip and ready:
            # every group's squares are in: one workgroup adds them up and leaves {norm, coefficient} on the device
            N.note_device(bufs["norm"].device)
            hyper0 = self._captured["hyper"][ready[0][0]] if capturing else None
            check(N.lib.ru3d_grad_norm_finish(ptr(bufs["partials"]), npartials, float(grad_scale), ptr(hyper0),
                                              self.max_grad_norm, ptr(bufs["norm"]), stream()), "grad_norm_finish")
            coef = bufs["norm"][1:]
            self.last_grad_norm = bufs["norm"][0]
        for gi, group, plan, step_no in ready:
            N.note_device(plan.table.device)
            if capturing:
                # the captured launch reads lr / bias corrections / grad_scale from the device block that
                # replay_scalars() refreshes in front of every replay
                self._captured["steps"][gi] = step_no - 1.0     # the first replay IS this step
                amp = self._captured.get("amp")
                if amp is not None:
                    # fp16: the device-side loss scaler decides (skip on overflow, 1 / scale, the true step number)
                    self._captured["amp_base"][gi] = step_no - 1.0
                    check(N.lib.ru3d_adam_multi_amp(ptr(plan.table), ptr(plan.block_map), plan.nblocks, _CHUNK,
                                                    ptr(self._captured["hyper"][gi]), ptr(amp), stream()), "adam_multi_amp")
                else:
                    self._launch_dev(plan, self._captured["hyper"][gi], coef)
                continue
            if self._captured is not None and gi in self._captured["steps"]:
                self._captured["steps"][gi] = step_no
                self._captured["amp_base"][gi] = step_no      # (the scaler re-uploads its block with steps = 0)
            self._launch(plan, group, step_no, float(grad_scale), coef)
        import _ops
        _ops.WEIGHTS_EPOCH[0] += 1      # packed copies of the weights are stale now
        return loss

    # ---- a training step captured in a hipGraph (graph.GraphedTrainStep)
    def begin_capture(self, hyper):
        """hyper: device float32 [len(param_groups), 8]; the captured update kernels read their scalars from it."""
        if hyper.shape != (len(self.param_groups), 8) or hyper.dtype != torch.float32:
            raise ValueError("begin_capture: hyper must be float32 [groups, 8]")
        self._captured = {"hyper": hyper, "steps": {}, "amp": None, "amp_base": {}}
        for gi, group in enumerate(self.param_groups):       # device-side plan pieces cannot be made while capturing
            if group["params"]:
                self._plan(gi, group, True)
        if self.max_grad_norm is not None and any(g["params"] for g in self.param_groups):
            self._clip_buffers(True)

    def end_capture(self):
        """Leave captured mode and drop what was allocated for it."""
        self._captured = None
        for key in [k for k in self._plans if k[1]]:       # (group, captured=True)
            del self._plans[key]
        self._clip.pop(True, None)           # the norm block stays: last_grad_norm keeps the last replay's value

    def replay_scalars(self, out, grad_scale=1.0):
        """Advance the step counts of the captured groups by one and write this step's scalars into `out` (CPU float32
        [groups, 8], the row of the subclass's `_row`) - the caller uploads them."""
        cap = self._captured
        cap["dirty"] = True
        for gi, step_no in cap["steps"].items():
            step_no += 1.0
            cap["steps"][gi] = step_no
            self._row(out[gi], self.param_groups[gi], step_no, grad_scale)

    def sync_captured_steps(self):
        """Write the step counts reached by graph replays back into state[p]['step'] (state_dict fidelity)."""
        cap = self._captured
        if cap is None or not cap.get("dirty"):
            return
        cap["dirty"] = False
        if not self._COUNTS_STEPS:
            return
        if cap.get("amp") is not None:
            # the device counted the steps that were not skipped (one 32-byte read-back, on demand only)
            taken = int(cap["amp"].view(torch.int32)[5].item())
            for gi in list(cap["steps"]):
                cap["steps"][gi] = cap["amp_base"].get(gi, 0.0) + taken
        for gi, step_no in cap["steps"].items():
            for p in self.param_groups[gi]["params"]:
                st = self.state.get(p)
                if st:
                    st["step"] = torch.tensor(float(step_no))

    def state_dict(self):
        self.sync_captured_steps()
        return super().state_dict()

    def load_state_dict(self, state_dict):
        """torch's layout; the step counts are kept on the HOST whatever device the checkpoint was mapped to (step() reads
        them every call: a device tensor there is a sync per step and cannot be read inside a graph capture)."""
        super().load_state_dict(state_dict)
        for st in self.state.values():
            if torch.is_tensor(st.get("step")) and st["step"].device.type != "cpu":
                st["step"] = st["step"].detach().to("cpu", torch.float32)


class _AdamFamily(_Fused):
    """torch.optim.Adam's state: {'step' (host float32), 'exp_avg', 'exp_avg_sq'}."""

    def _slots(self, p, group, capturing):
        st = self.state[p]
        if len(st) == 0:
            if capturing:
                raise N.Ru3dError("optim.%s: take one eager step before capturing (the moment buffers are "
                                  "created and zeroed by the first step)" % self._NAME)
            st["step"] = torch.tensor(0.0)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return st["exp_avg"], st["exp_avg_sq"]

    def _check_group(self, group):
        if group.get("amsgrad") or group.get("maximize"):
            raise N.Ru3dError("optim.%s: amsgrad / maximize are not implemented" % self._NAME)


class Adam(_AdamFamily):
    _NAME = "Adam"

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, max_grad_norm=None):
        if weight_decay != 0 or amsgrad:
            raise ValueError("ru3d optim.Adam implements plain Adam (weight_decay=0, amsgrad=False)")
        if lr < 0 or eps < 0 or not (0 <= betas[0] < 1 and 0 <= betas[1] < 1):
            raise ValueError("invalid Adam hyper-parameters")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=0, amsgrad=False), max_grad_norm)

    def captures_with_scaler(self):
        return self.max_grad_norm is None

    def _launch(self, plan, group, step_no, grad_scale, coef):
        b1, b2 = group["betas"]
        # a null coefficient is the unclipped step: ru3d_adam_multi's kernel and bits
        check(N.lib.ru3d_adam_multi_clip(ptr(plan.table), ptr(plan.block_map), plan.nblocks, _CHUNK,
                                         float(group["lr"]), float(b1), float(b2), float(group["eps"]),
                                         1.0 - b1 ** step_no, 1.0 - b2 ** step_no, float(grad_scale), ptr(coef), stream()),
              "adam_multi_clip")

    def _launch_dev(self, plan, hyper_row, coef):
        check(N.lib.ru3d_adam_multi_clip_dev(ptr(plan.table), ptr(plan.block_map), plan.nblocks, _CHUNK,
                                             ptr(hyper_row), ptr(coef), stream()), "adam_multi_clip_dev")

    def _row(self, row, group, step_no, grad_scale):
        """lr, beta1, beta2, eps, bias_corr1, bias_corr2, grad_scale, sqrt(bias_corr2)"""
        b1, b2 = group["betas"]
        row[0] = group["lr"]; row[1] = b1; row[2] = b2; row[3] = group["eps"]
        row[4] = 1.0 - b1 ** step_no; row[5] = 1.0 - b2 ** step_no; row[6] = grad_scale
        row[7] = float(row[5]) ** 0.5     # sqrt of the float32 bias_corr2, as ru3d_adam_multi takes it on the host
        if self._captured.get("amp") is not None:
            # device-side loss scaler: the kernel derives the step number from the steps really taken (skips are
            # decided on the device); slot 5 carries the count before the capture as an int32
            gi = next(i for i, g in enumerate(self.param_groups) if g is group)
            row[5:6].view(torch.int32)[0] = int(self._captured["amp_base"].get(gi, 0.0))
            row[4] = b1 - float(torch.tensor(b1, dtype=torch.float32))      # residuals: beta = float32 value + this
            row[7] = b2 - float(torch.tensor(b2, dtype=torch.float32))


class AdamW(_AdamFamily):
    """torch.optim.AdamW: decoupled weight decay p *= 1 - lr * weight_decay in front of Adam's update."""
    _NAME = "AdamW"

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False,
                 max_grad_norm=None):
        if not 0.0 <= lr:
            raise ValueError("Invalid learning rate: {}".format(lr))
        if not 0.0 <= eps:
            raise ValueError("Invalid epsilon value: {}".format(eps))
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError("Invalid beta parameter at index 0: {}".format(betas[0]))
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError("Invalid beta parameter at index 1: {}".format(betas[1]))
        if not 0.0 <= weight_decay:
            raise ValueError("Invalid weight_decay value: {}".format(weight_decay))
        if amsgrad:
            raise ValueError("ru3d optim.AdamW does not implement amsgrad")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False),
                         max_grad_norm)

    def _launch(self, plan, group, step_no, grad_scale, coef):
        b1, b2 = group["betas"]
        check(N.lib.ru3d_adamw_multi(ptr(plan.table), ptr(plan.block_map), plan.nblocks, _CHUNK,
                                     float(group["lr"]), float(b1), float(b2), float(group["eps"]),
                                     float(group["weight_decay"]), 1.0 - b1 ** step_no, 1.0 - b2 ** step_no,
                                     float(grad_scale), ptr(coef), stream()), "adamw_multi")

    def _launch_dev(self, plan, hyper_row, coef):
        check(N.lib.ru3d_adamw_multi_dev(ptr(plan.table), ptr(plan.block_map), plan.nblocks, _CHUNK,
                                         ptr(hyper_row), ptr(coef), stream()), "adamw_multi_dev")

    def _row(self, row, group, step_no, grad_scale):
        """lr, beta1, beta2, eps, bias_corr1, bias_corr2, grad_scale, weight_decay (the kernel takes sqrt(bias_corr2))"""
        b1, b2 = group["betas"]
        row[0] = group["lr"]; row[1] = b1; row[2] = b2; row[3] = group["eps"]
        row[4] = 1.0 - b1 ** step_no; row[5] = 1.0 - b2 ** step_no; row[6] = grad_scale
        row[7] = group["weight_decay"]


class SGD(_Fused):
    """torch.optim.SGD with dampening = 0: momentum, Nesterov momentum, (coupled) weight decay.  state[p] =
    {'momentum_buffer'} as in torch, no entry when momentum == 0."""
    _NAME = "SGD"
    _COUNTS_STEPS = False

    def __init__(self, params, lr, momentum=0, dampening=0, weight_decay=0, nesterov=False, max_grad_norm=None):
        if lr < 0.0:
            raise ValueError("Invalid learning rate: {}".format(lr))
        if momentum < 0.0:
            raise ValueError("Invalid momentum value: {}".format(momentum))
        if weight_decay < 0.0:
            raise ValueError("Invalid weight_decay value: {}".format(weight_decay))
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        if dampening != 0:
            raise ValueError("ru3d optim.SGD does not implement dampening")
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=0, weight_decay=weight_decay,
                                      nesterov=bool(nesterov)), max_grad_norm)

    def _check_group(self, group):
        if group.get("dampening", 0) != 0 or group.get("maximize"):
            raise N.Ru3dError("optim.SGD: dampening / maximize are not implemented")
        if group["nesterov"] and group["momentum"] <= 0:
            raise N.Ru3dError("optim.SGD: Nesterov momentum requires a momentum")

    def _slots(self, p, group, capturing):
        if group["momentum"] == 0:
            return None, None
        st = self.state[p]
        if st.get("momentum_buffer") is None:
            if capturing:
                raise N.Ru3dError("optim.SGD: take one eager step before capturing (the momentum buffers are created "
                                  "and zeroed by the first step)")
            # zero, not torch's clone of the first d: momentum * 0 + d is d, bit for bit
            st["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return st["momentum_buffer"], None

    def _launch(self, plan, group, step_no, grad_scale, coef):
        check(N.lib.ru3d_sgd_multi(ptr(plan.table), ptr(plan.block_map), plan.nblocks, _CHUNK,
                                   float(group["lr"]), float(group["momentum"]), float(group["weight_decay"]),
                                   int(bool(group["nesterov"])), float(grad_scale), ptr(coef), stream()), "sgd_multi")

    def _launch_dev(self, plan, hyper_row, coef):
        check(N.lib.ru3d_sgd_multi_dev(ptr(plan.table), ptr(plan.block_map), plan.nblocks, _CHUNK,
                                       ptr(hyper_row), ptr(coef), stream()), "sgd_multi_dev")

    def _row(self, row, group, step_no, grad_scale):
        """lr, momentum, weight_decay, nesterov (0 / 1), -, -, grad_scale, -"""
        row[0] = group["lr"]; row[1] = group["momentum"]; row[2] = group["weight_decay"]
        row[3] = 1.0 if group["nesterov"] else 0.0
        row[4] = 0.0; row[5] = 0.0; row[6] = grad_scale; row[7] = 0.0


_CLIP_TABLES = {}      # (device, numels) -> table + partials of clip_grad_norm_; a few small entries, dropped beyond eight


def clip_grad_norm_(parameters, max_norm):
    """torch.nn.utils.clip_grad_norm_(parameters, max_norm) (norm_type 2, error_if_nonfinite=False) for float32 gradients
    on a HIP device: the gradients are scaled in place by min(1, max_norm / (norm + 1e-6)) and the norm comes back as a
    0-dim device tensor.  Three launches, a fixed summation order, no host synchronisation."""
    if torch.is_tensor(parameters):
        parameters = [parameters]
    params = [p for p in parameters if p.grad is not None]
    max_norm = _check_max_grad_norm(max_norm)
    if max_norm is None:
        raise ValueError("clip_grad_norm_: max_norm is required")
    if not params:
        return torch.zeros(())
    dev = params[0].grad.device
    for p in params:
        N.require_device(p.grad, "gradient")
        if p.grad.device != dev:
            raise N.Ru3dError("clip_grad_norm_: gradients must share one device")
    key = (dev,) + tuple(p.numel() for p in params)      # all that the block map and the table's size depend on
    entry = _CLIP_TABLES.get(key)
    if entry is None:
        if len(_CLIP_TABLES) >= 8:
            _CLIP_TABLES.clear()
        entry = _CLIP_TABLES[key] = {"table": _GradTable("clip_grad_norm_")}
    tab = entry["table"]
    tab.update(params)
    if entry.get("partials") is None or entry["partials"].numel() != tab.nblocks:
        entry["partials"] = torch.empty(tab.nblocks, dtype=torch.float64, device=dev)
    out = torch.empty(2, dtype=torch.float32, device=dev)      # a fresh block: the returned norm stays valid
    N.note_device(dev)
    check(N.lib.ru3d_grad_norm(ptr(tab.table), ptr(tab.block_map), tab.nblocks, _CHUNK, ptr(entry["partials"]), 1.0,
                               max_norm, ptr(out), stream()), "grad_norm")
    check(N.lib.ru3d_grad_scale_dev(ptr(tab.table), ptr(tab.block_map), tab.nblocks, _CHUNK, ptr(out[1:]), stream()),
          "grad_scale_dev")
    return out[0]


class _GradTable(_Table):
    """A _Table of (grad pointer, count) rows, one per parameter, refilled when the gradient tensors move (GradSync
    re-aliases them into its buckets; autograd allocates fresh ones otherwise)."""

    def __init__(self, who="LossScaler"):
        super().__init__()
        self.who = who
        self.key = None         # what the device table was last filled from: the device, (grad pointer, count) per row

    def update(self, params, capturing=False, refill=False):
        """refill: fill and copy even when nothing moved (a captured step: the copy has to be a node of ITS graph)."""
        grads = [p.grad for p in params]
        dev = next(g.device for g in grads if g is not None)
        key = (dev,) + tuple((0 if g is None else g.data_ptr(), p.numel()) for p, g in zip(params, grads))
        if key == self.key and not refill:
            return
        for g in grads:
            if g is not None and (g.dtype != torch.float32 or not g.is_contiguous()):
                raise N.Ru3dError("%s: gradients must be contiguous float32" % self.who)
        self.prepare([p.numel() for p in params], dev)
        self.fill([(None, None if g is None else g.data_ptr(), None, None, p.numel()) for p, g in zip(params, grads)],
                  capturing)
        self.key = key


class LossScaler:
    """Dynamic loss scaling for fp16 storage - the reference's apex O1 behaviour (trainer.py:492-493 `amp.scale_loss`,
    538-542 `amp.initialize(..., opt_level)`): start at 2**16, skip the optimizer step and halve the scale when a
    gradient overflows, double it after `growth_interval` (2000) clean steps, up to 2**24 (apex's max_loss_scale).

        scaler = optim.LossScaler()
        scaler.scale(loss).backward()
        scaler.step(optimizer)        # unscale + inf/nan check on the device, one 4-byte read-back, step or skip

    With optim.Adam / AdamW / SGD the 1/scale factor is applied inside the fused update kernel (and in the gradient norm
    of max_grad_norm, which is then the norm of the true gradients); any other torch optimizer gets its gradients
    unscaled in place first.  bf16 storage needs none of this."""

    def __init__(self, init_scale=65536.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000,
                 min_scale=2.0 ** -24, max_scale=2.0 ** 24):
        self.loss_scale = float(init_scale)
        self.growth_factor, self.backoff_factor = float(growth_factor), float(backoff_factor)
        self.growth_interval = int(growth_interval)
        self.min_scale = float(min_scale)
        self.max_scale = float(max_scale)      # apex: max_loss_scale = 2.**24
        self.growth_tracker = 0
        self.skipped_steps = 0
        self._scale_t = None
        self._found = None
        self._tables = {}
        self._dev = None            # captured mode: the ru3d_amp_state block (uint8[32]) on the device
        self._dev_skipped = 0       # its `skipped` count at the last sync

    # ---- captured mode (graph.GraphedTrainStep): the scaler state lives on the device, see ru3d_amp_state
    def begin_capture(self, optimizer, device):
        """Move the state into a device block and tell optim.Adam to take its decisions from there.  Call after
        optimizer.begin_capture()."""
        if not isinstance(optimizer, _Fused) or not optimizer.captures_with_scaler() or optimizer._captured is None:
            raise TypeError("LossScaler.begin_capture needs an optim.Adam without max_grad_norm that is being captured "
                            "(ru3d_adam_multi_amp is the one update kernel that follows the device-side scaler)")
        self._dev = torch.zeros(32, dtype=torch.uint8, device=device)
        self._upload()
        for gi, group in enumerate(optimizer.param_groups):
            if group["params"]:
                self._tables.setdefault((id(optimizer), gi, "cap"), _GradTable()).prepare(
                    [p.numel() for p in group["params"]], device)
        self._scale_t = self._dev[0:4].view(torch.float32).view(())
        self._found = self._dev[8:12].view(torch.float32)
        optimizer._captured["amp"] = self._dev

    def _upload(self):
        f = torch.zeros(8, dtype=torch.float32)
        i = f.view(torch.int32)
        f[0], f[1], f[2] = self.loss_scale, 1.0 / self.loss_scale, 0.0
        i[3], i[4] = self.growth_tracker, 0
        i[5] = 0
        self._dev.copy_(f.view(torch.uint8))
        self._dev_skipped = 0

    def sync(self):
        """Captured mode: read the device block back into the host-side fields (one 32-byte copy; state_dict, logging)."""
        if self._dev is None:
            return
        f = self._dev.cpu().view(torch.float32)
        i = f.view(torch.int32)
        self.loss_scale = float(f[0])
        self.growth_tracker = int(i[3])
        self.skipped_steps += int(i[4]) - self._dev_skipped
        self._dev_skipped = int(i[4])

    def eager_step(self, optimizer, loss):
        """One eager step (a batch of another shape) between replays: the state comes back to the host for it and returns
        to the device block afterwards."""
        dev = self._dev
        self.sync()
        optimizer.sync_captured_steps()
        # _upload() below restarts the device's count of steps taken at 0, whether or not this step is skipped: the base
        # it is added to moves up to the count reached now (amp_base + device steps == updates applied, always)
        cap = optimizer._captured
        if cap is not None:
            for gi in cap["steps"]:
                cap["amp_base"][gi] = cap["steps"][gi]
        self._dev = None
        self._scale_t = self._found = None
        try:
            self.scale(loss).backward()
            return self.step(optimizer)
        finally:
            self._dev = dev
            self._upload()
            self._scale_t = dev[0:4].view(torch.float32).view(())
            self._found = dev[8:12].view(torch.float32)

    def end_capture(self):
        self.sync()
        self._dev = None
        self._scale_t = None
        self._found = None

    def scale(self, loss):
        if self._scale_t is None or self._scale_t.device != loss.device:
            self._scale_t = torch.full((), self.loss_scale, dtype=torch.float32, device=loss.device)
            self._found = torch.zeros(1, dtype=torch.float32, device=loss.device)
        return loss * self._scale_t

    def step(self, optimizer):
        """Returns True when the optimizer stepped, False when the step was skipped because of an overflow."""
        if self._scale_t is None:
            raise RuntimeError("LossScaler.step() before LossScaler.scale(loss).backward()")
        fused = isinstance(optimizer, _Fused)      # Adam, AdamW, SGD: 1 / scale goes into the update (and norm) kernels
        if self._dev is not None:
            if not torch.cuda.is_current_stream_capturing():
                raise RuntimeError("LossScaler: an eager step while the scaler is in captured mode (end_capture() first)")
            # captured: check -> Adam (skips itself on overflow) -> scaler update, all decided on the device
            for gi, group in enumerate(optimizer.param_groups):
                params = [p for p in group["params"]]
                if not any(p.grad is not None for p in params):
                    continue
                tab = self._tables.setdefault((id(optimizer), gi, "cap"), _GradTable())
                tab.update(params, capturing=True, refill=True)
                N.note_device(tab.table.device)
                check(N.lib.ru3d_grad_scale_check(ptr(tab.table), ptr(tab.block_map), tab.nblocks, _CHUNK, 1.0,
                                                  ptr(self._found), stream()), "grad_scale_check")
            optimizer.step()
            check(N.lib.ru3d_amp_update(ptr(self._dev), self.growth_factor, self.backoff_factor, self.growth_interval,
                                        self.min_scale, self.max_scale, stream()), "amp_update")
            return None
        inv = 1.0 / self.loss_scale
        self._found.zero_()
        any_grad = False
        for gi, group in enumerate(optimizer.param_groups):
            params = [p for p in group["params"]]
            if not any(p.grad is not None for p in params):
                continue
            any_grad = True
            tab = self._tables.setdefault((id(optimizer), gi), _GradTable())
            tab.update(params)
            N.note_device(tab.table.device)
            check(N.lib.ru3d_grad_scale_check(ptr(tab.table), ptr(tab.block_map), tab.nblocks, _CHUNK,
                                              1.0 if fused else inv, ptr(self._found), stream()), "grad_scale_check")
        overflow = any_grad and bool(self._found.item() != 0.0)      # the one host read-back of the fp16 step
        if overflow:
            self.loss_scale = max(self.loss_scale * self.backoff_factor, self.min_scale)
            self.growth_tracker = 0
            self.skipped_steps += 1
        else:
            if fused:
                optimizer.step(grad_scale=inv)
            else:
                optimizer.step()
            self.growth_tracker += 1
            if self.growth_tracker >= self.growth_interval:
                self.loss_scale = min(self.loss_scale * self.growth_factor, self.max_scale)
                self.growth_tracker = 0
        self._scale_t.fill_(self.loss_scale)
        return not overflow

    def state_dict(self):
        """apex's `amp.state_dict()` layout, which the reference checkpoints as 'amp_state_dict' (trainer.py:617-618):
        {'loss_scaler0': {'loss_scale': float, 'unskipped': int}} - `unskipped` is apex's name for the count of clean
        steps since the last change of the scale.  The extra key 'ru3d' (skipped-step count, dtype tag) is ignored by
        apex's loader, which reads only the loss_scaler<i> entries."""
        self.sync()
        return {"loss_scaler0": {"loss_scale": self.loss_scale, "unskipped": self.growth_tracker},
                "ru3d": {"dtype": "fp16", "skipped_steps": self.skipped_steps}}

    def load_state_dict(self, state):
        """Reads the apex layout (a checkpoint of the reference) and this class's round-2 flat layout."""
        if not isinstance(state, dict):
            return
        if isinstance(state.get("loss_scaler0"), dict):
            inner = state["loss_scaler0"]
            self.loss_scale = float(inner["loss_scale"])
            self.growth_tracker = int(inner.get("unskipped", 0))
            extra = state.get("ru3d")
            self.skipped_steps = int(extra.get("skipped_steps", 0)) if isinstance(extra, dict) else 0
        elif "loss_scale" in state:
            self.loss_scale = float(state["loss_scale"])
            self.growth_tracker = int(state.get("growth_tracker", 0))
            self.skipped_steps = int(state.get("skipped_steps", 0))
        else:
            return
        self.loss_scale = min(max(self.loss_scale, self.min_scale), self.max_scale)
        if self._scale_t is not None:
            self._scale_t.fill_(self.loss_scale)
