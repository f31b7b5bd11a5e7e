"""Drop-in `loss` module: Dice / DiceLoss / FocalLoss / HybirdLoss on the fused HIP loss kernels.

Import surface of the reference `loss.py` (functions `logits`, `flatten_and_tranpose_C`, `dice`,
`focal_loss`; classes `Dice`, `DiceLoss`, `FocalLoss`, `HybirdLoss`) plus the legacy aliases the
older training scripts import (`DiceCoef`, `FocalDiceCoefLoss`: reference nb_train_KITS19.py:4,
run_train.py:2 - no implementation of either name survives in the reference, so their semantics
here are this build's choice: `DiceCoef(weight=w) == Dice(weight_v=w)`,
`FocalDiceCoefLoss(d_weight=w) == HybirdLoss(weight_v=w)`).

Each module call is ONE fused forward pass over (logits, labels) on the device plus an on-device
finalize - no one-hot tensor, no per-class Python loop, no host synchronisation (the reference
syncs C+2 times per call, loss.py:231,241,246).  The returned value is a 0-dim tensor on the
logits' device that supports .backward(), .item() and torch.isnan like the reference's.

Bug-compatible behaviour kept (reference loss.py:68-69, 154-155, 236-237): `weight_c` and the
class-presence mask are accepted and have no effect; weights are `weight_v / sum|weight_v|`.
Labels outside [0, C) raise `RuntimeError("Class values must be smaller than num_classes.")` like the
reference's F.one_hot (loss.py:27) - without a host synchronisation of their own: the forward kernel
counts them into its state block, those 4 bytes ride to pinned host memory behind the kernel, and
`raise_on_bad_labels()` - called by the next loss call and by `Trainer` right after its own read-back of
the loss scalars - raises as soon as that copy has landed (the loss value of such a step is NaN).
`check_labels=True` / RU3D_CHECK_LABELS=1 checks before the launch instead (one sync per call).  With
C == 1 the reference only works for all-zero targets and so does this.

Beyond the reference: nested or overlapping structures train one sigmoid channel per group of label values with
`GroupHybirdLoss` / `GroupDiceLoss` / `GroupFocalLoss` / `GroupDice` (the section "overlapping label groups" below).
`TopKLoss` / `HybirdTopKLoss` (the section "top-k cross-entropy" at the end) are nnU-Net's top-k cross-entropy and its
`DC_and_topk_loss`: the cross-entropy averaged over the hardest k percent of the batch's voxels, selected on the device
between the forward and the backward.  `DeepSupervisionLoss` does not take them as a base: top-k under deep supervision
is not implemented.

Partly annotated cases: `Dice`, `DiceLoss`, `FocalLoss`, `HybirdLoss`, `TopKLoss` and `HybirdTopKLoss` take
`ignore_label=` (default None: nothing changes), `DeepSupervisionLoss` takes it over from its base.  The loss is then the
loss of the voxels whose label is not `ignore_label`; those voxels count in no sum, their logits are never read and
their gradient is exactly 0 (the section "ignore label" below).
"""
import collections
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

import _native as N
from _native import check, ptr, stream

_CHECK_LABELS = os.environ.get("RU3D_CHECK_LABELS", "0") == "1"


# --------------------------------------------------------------------------- functional helpers (API parity)
def logits(input):
    """(N, C, d1, ..., dn) -> class probabilities: softmax over C, sigmoid when C == 1."""
    return torch.softmax(input, dim=1) if input.size(1) > 1 else torch.sigmoid(input)


def flatten_and_tranpose_C(input, target):
    """(N, C, d1..dn), (N, d1..dn) -> (N*d1*..*dn, C) scores and int64 one-hot."""
    c = input.size(1)
    flat = input.reshape(input.size(0), c, -1).transpose(1, 2).reshape(-1, c)
    return flat, F.one_hot(target, num_classes=c).reshape(-1, c)


def dice(input, target, alpha=0.5, beta=0.5, smooth=1e-7):
    """Tversky index of two same-shaped tensors (probabilities or masks).  Device tensors go through
    the HIP reduction kernel; host tensors (trainer.evaluate_case works on numpy-derived CPU masks)
    are reduced by torch on the host - that evaluation path is not part of the training hot path."""
    if input.is_cuda:
        p = input.detach().reshape(-1).float().contiguous()
        g = target.detach().reshape(-1).float().contiguous()
        out = torch.empty((), dtype=torch.float32, device=p.device)
        N.note_device(p.device)
        # ru3d_tversky's layout: one row of three float64 sums per block of 2048 elements, at most 1024 blocks
        ws = N.workspace(min((p.numel() + 2047) // 2048, 1024) * 3 * 8, p.device)
        check(N.lib.ru3d_tversky(ptr(p), ptr(g), p.numel(), alpha, beta, smooth, ptr(out), ptr(ws), ws.numel(),
                                 stream()), "tversky")
        return out
    p = input.reshape(-1)
    g = target.reshape(-1)
    tp = (p * g).sum()
    fn = ((1 - p) * g).sum()
    fp = (p * (1 - g)).sum()
    return (tp + smooth) / (tp + alpha * fn + beta * fp + smooth)


# --------------------------------------------------------------------------- deferred label check
_FLAG_RING = 64
_flag_host = {}                       # device -> [pinned int32 ring, next slot, events per slot]
_pending = collections.deque()        # (event, pinned ring, slot) in launch order
_BAD_LABELS = "Class values must be smaller than num_classes."      # F.one_hot's message (reference loss.py:27)


# graph.GraphedTrainStep sets this to a list while it captures a step: the state blocks of the captured loss calls, whose
# counts it then reads back after every replay (a copy queued OUTSIDE the graph, into the same pinned ring)
CAPTURE_SINK = [None]


def _note_label_flag(state):
    """Queue the D2H copy of the forward kernel's out-of-range label count (4 bytes, stream-ordered, no sync)."""
    dev = state.device
    if torch.cuda.is_current_stream_capturing():
        if CAPTURE_SINK[0] is not None:
            CAPTURE_SINK[0].append(state)
        return
    ent = _flag_host.get(dev)
    if ent is None:
        ent = _flag_host[dev] = [torch.zeros(_FLAG_RING, dtype=torch.int32).pin_memory(), 0, [None] * _FLAG_RING]
    ring, slot, events = ent
    if events[slot] is not None:
        events[slot].synchronize()      # 64 loss calls behind: long done
        raise_on_bad_labels()
    off = _BAD_OFF[0]
    ring[slot:slot + 1].copy_(state[off:off + 4].view(torch.int32), non_blocking=True)
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream(dev))
    events[slot] = ev
    _pending.append((ev, ring, slot, events))
    ent[1] = (slot + 1) % _FLAG_RING


def raise_on_bad_labels(wait=False):
    """Raise F.one_hot's error for every finished loss call that saw a label outside [0, C).  Never blocks unless
    `wait`: call it right after a read-back of the loss (`.item()`, `.cpu()`) to learn about that very step."""
    while _pending:
        ev, ring, slot, events = _pending[0]
        if wait:
            ev.synchronize()
        elif not ev.query():
            return
        _pending.popleft()
        if events[slot] is ev:
            events[slot] = None
        if int(ring[slot]) > 0:
            _pending.clear()
            raise RuntimeError(_BAD_LABELS)


_BAD_OFF = [int(N.lib.ru3d_loss_state_bad_labels_offset())]


# --------------------------------------------------------------------------- fused loss
def _flat_strides(x):
    """(stride_n, stride_c, stride_v) of an (N, C, *spatial) tensor whose spatial dims collapse to one
    axis with a single stride (true for NCDHW-contiguous and for NDHWC tensors); None otherwise."""
    sizes, strides = x.shape[2:], x.stride()[2:]
    sv = None
    expect = None
    for size, stride in zip(reversed(sizes), reversed(strides)):
        if size == 1:
            continue
        if sv is None:
            sv, expect = stride, stride * size
        else:
            if stride != expect:
                return None
            expect = stride * size
    if sv is None:
        sv = 1
    return x.stride(0), x.stride(1), sv


# --------------------------------------------------------------------------- ignore label
# The loss with an ignore label is the loss applied to the counted voxels alone: gather the voxels whose label is not
# ignore_label into one (1, C, M) batch and call the plain loss on it.  With S those voxels - over the whole batch - and
# M = |S|: tp_c, sp_c, sg_c run over S only (an ignored voxel adds to no sum, not to sp either), the Tversky formula is
# unchanged; focal_c = C * (sum over S of -(1-p_c)^gamma g_c log p_c) / max(M, 1); d loss / d logits is exactly 0.0 at an
# ignored voxel, whose logits influence nothing (they may be NaN or Inf: padding).  M = 0 gives dice_c = 1: DiceLoss,
# FocalLoss, HybirdLoss 0 and Dice sum w, gradient all zeros.  A label outside [0, C) that is not the ignore label is a
# bad label as ever.  Deep supervision: a level's voxel is ignored iff the label it reads is, and every level divides by
# its own max(M_l, 1).  Top-k follows nnU-Net (ignore_index in the cross-entropy, then top-k over ALL voxels): an ignored
# voxel has ce = 0 and takes part in the selection like any voxel whose cross-entropy is 0; K = max(1, int(N V k / 100))
# stays relative to all voxels - a K relative to M would have to be computed on the device, which is not implemented.
def _checked_softmax_ignore(ignore_label, c, target):
    """The ignore label of one call as an int (None: none), or ValueError - before anything is launched."""
    if ignore_label is None:
        return None
    ig = int(ignore_label)
    if c == 1:
        raise ValueError("ignore_label: not with C == 1 (the sigmoid form); GroupHybirdLoss is the single-channel loss "
                         "with an ignore label")
    if 0 <= ig < c:
        raise ValueError("ignore_label %d lies inside the class range [0, %d)" % (ig, c))
    if target.dtype == torch.uint8 and not 0 <= ig <= 255:
        raise ValueError("ignore_label %d cannot occur in uint8 labels" % ig)
    if not -2 ** 31 <= ig < 2 ** 31:
        raise ValueError("ignore_label %d is no int32 value" % ig)
    return ig


def _view(x, st, lab, lab_code):
    """How every entry point begins: logits, stride_n, stride_c, stride_v, labels, label_dtype."""
    return ptr(x), st[0], st[1], st[2], ptr(lab), lab_code


class _Operands:
    """What _loss_operands prepares.  x, st: the float32 logits and their flat strides (tuples of them, one per level,
    when a list of logits came in, and no view then); checked: the labels were range-checked before the launch.  A ctx
    keeps x and lab by save_for_backward and meta() beside them; its backward makes the _view of those again."""
    __slots__ = ("x", "lab", "st", "lab_code", "n", "c", "v", "checked", "view", "ignore")

    def __init__(self, x, lab, st, lab_code, n, c, v, checked, ignore=None):
        self.x, self.lab, self.st, self.lab_code = x, lab, st, lab_code
        self.n, self.c, self.v, self.checked = n, c, v, checked
        self.ignore = ignore      # the call's checked ignore label (None: the plain entry points)
        self.view = None if isinstance(x, tuple) else _view(x, st, lab, lab_code)

    def meta(self):
        return self.st, self.lab_code, self.n, self.v, self.c


def _flat_logits(x):
    """Detached float32 logits whose spatial dims share one stride (a copy only where they do not), and the strides."""
    x = x.detach()
    if x.dtype != torch.float32:
        x = x.float()
    st = _flat_strides(x)
    if st is None:
        x = x.contiguous()
        st = _flat_strides(x)
    return x, st


def _label_operand(target):
    """Contiguous int64 / uint8 labels and their ABI code; any other dtype goes to int64."""
    if target.dtype in (torch.int64, torch.uint8):
        lab = target.contiguous()
    else:
        lab = target.long().contiguous()
    return lab, (N.LABEL_U8 if lab.dtype == torch.uint8 else N.LABEL_I64)


def _operand_parts(input, target, check_labels, one_hot, ignore=None):
    """What every fused loss does to its operands before it launches: float32 logits with a single spatial stride,
    contiguous int64 / uint8 labels, and the blocking label check where one is asked for.  input: one (N, C, d1, ..., dn)
    tensor, or - deep supervision - the list of the levels' tensors, finest first: the labels belong to the first, and x
    and st come back as tuples.  one_hot=False (the group losses): the labels are no class indices of the C channels, so
    neither that check nor the C == 1 rule applies; check_labels then says that the caller has checked them itself.
    ignore: the blocking check skips this value, as _GroupLossFn's does."""
    many = isinstance(input, (list, tuple))
    first = input[0] if many else input
    N.require_device(first, "loss input")
    if target.device != first.device:
        raise N.Ru3dError("loss: target is on %s but input on %s" % (target.device, first.device))
    if first.dim() < 2:
        raise N.Ru3dError("loss: input must be (N, C, d1, ..., dn)")
    n, c = first.shape[0], first.shape[1]
    if c > N.MAX_CLASSES:
        raise N.Ru3dError("loss: %d classes (max %d)" % (c, N.MAX_CLASSES))
    if tuple(target.shape) != (n,) + tuple(first.shape[2:]):
        raise N.Ru3dError("loss: target shape %s does not match input %s" % (tuple(target.shape),
                                                                             tuple(first.shape)))
    x, st = zip(*[_flat_logits(level) for level in input]) if many else _flat_logits(input)
    v = 1
    for s in first.shape[2:]:
        v *= s
    lab, lab_code = _label_operand(target)
    checked = bool(check_labels or (one_hot and c == 1))
    if one_hot and checked:
        # reference: F.one_hot(target, C) raises for labels >= C (always hit by C == 1 with labels {0,1})
        seen = lab if ignore is None else lab[lab != ignore]
        if seen.numel() and (int(seen.max()) >= c or int(seen.min()) < 0):
            raise RuntimeError(_BAD_LABELS)
    return x, lab, st, lab_code, n, c, v, checked


def _loss_operands(input, target, check_labels, one_hot=True, ignore=None):
    """_operand_parts as the object the shared helpers take."""
    return _Operands(*_operand_parts(input, target, check_labels, one_hot, ignore), ignore)


def _ignore_args(ignore):
    """(has_ignore, ignore_label) as the ..._ignore_... entry points take them."""
    return 1, ignore


def _weight_array(weight_v, c):
    if weight_v is None:
        return None
    if len(weight_v) != c:
        raise RuntimeError("weight_v has %d entries for %d classes" % (len(weight_v), c))
    return (N.ctypes.c_float * c)(*[float(w) for w in weight_v])


def _forward_scaffold(dev, state_bytes, ws_bytes, weight_v, c, verdict=True):
    """What every forward does between its operands and its ABI call: an earlier call's verdict on its labels, if it has
    landed (no wait; verdict=False: the second leg of a mixed loss, whose first has asked); a state block and the 0-dim
    float32 output; the workspace; weight_v as the pointer the ABI takes (None: all ones)."""
    if verdict:
        raise_on_bad_labels()
    state = torch.empty(state_bytes, dtype=torch.uint8, device=dev)
    out = torch.empty((), dtype=torch.float32, device=dev)
    ws = N.workspace(ws_bytes, dev)
    wv = _weight_array(weight_v, c)
    return state, out, ws, (N.ctypes.cast(wv, N.ctypes.c_void_p) if wv is not None else None)


def _note_state(ops, state, other=None, offset=None):
    """The one rule of the deferred label check: a forward whose labels were not checked before the launch queues the
    read-back of its count, from `state`, or from `other` where state is None (a mixed loss: its Hybird leg's state
    where it has one, else its own).  offset: where the state keeps the count, when not where ru3d_loss_fwd's does (deep
    supervision: inside level 0's block)."""
    if ops.checked:
        return
    if state is None:
        state = other
    _note_label_flag(state if offset is None else state[offset - _BAD_OFF[0]:])


def _upstream(gout, dev):
    """The upstream gradient of a 0-dim loss as one contiguous float32 on dev."""
    g = gout.detach()
    if g.dtype != torch.float32 or g.device != dev:
        g = g.to(device=dev, dtype=torch.float32)
    N.note_device(dev)
    return g.reshape(1).contiguous()


def _empty_grad(x):
    """An uninitialised gradient with the strides of the logits x."""
    dz = torch.empty_like(x)   # preserve_format: same (dense) strides as the logits
    if dz.stride() != x.stride():
        dz = torch.empty_strided(x.shape, x.stride(), dtype=x.dtype, device=x.device)
    return dz


def _backward_prologue(gout, x):
    """(g, dz) of a backward: _upstream and _empty_grad (deep supervision takes the one once and the other per level)."""
    return _upstream(gout, x.device), _empty_grad(x)


def _backward_epilogue(dz, in_dtype, others=None):
    """dz rounded once to the logits' dtype.  With `others`: what a Function whose first input is the logits returns -
    that gradient, then None for each of its other inputs."""
    if in_dtype != torch.float32:
        dz = dz.to(in_dtype)
    return dz if others is None else (dz,) + (None,) * others


def _hybird_forward(ops, kind, gamma, weight_v, alpha, beta, smooth):
    """ru3d_loss_fwd of `kind` on prepared operands -> (state, 0-dim loss)."""
    state, out, ws, wv = _forward_scaffold(ops.x.device, N.lib.ru3d_loss_state_bytes(ops.c),
                                           N.lib.ru3d_loss_workspace_bytes(ops.n, ops.v, ops.c), weight_v, ops.c)
    if ops.ignore is None:
        check(N.lib.ru3d_loss_fwd(*ops.view, ops.n, ops.v, ops.c, kind, float(gamma), wv, float(alpha),
                                  float(beta), float(smooth), ptr(state), ptr(out), ptr(ws), ws.numel(), stream()),
              "loss_fwd")
    else:
        check(N.lib.ru3d_loss_ignore_fwd(*ops.view, ops.n, ops.v, ops.c, *_ignore_args(ops.ignore), kind, float(gamma),
                                         wv, float(alpha), float(beta), float(smooth), ptr(state), ptr(out), ptr(ws),
                                         ws.numel(), stream()), "loss_fwd")
    return state, out


def _hybird_backward(view, n, v, c, gamma, state, g, dz, ignore=None):
    """ru3d_loss_bwd: dz = g * d loss / d logits from the state a _hybird_forward left."""
    if ignore is None:
        check(N.lib.ru3d_loss_bwd(*view, n, v, c, gamma, ptr(state), ptr(g), ptr(dz), N.F32, stream()), "loss_bwd")
    else:
        check(N.lib.ru3d_loss_ignore_bwd(*view, n, v, c, *_ignore_args(ignore), gamma, ptr(state), ptr(g), ptr(dz),
                                         N.F32, stream()), "loss_bwd")


class _FusedLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, input, target, kind, gamma, weight_v, alpha, beta, smooth, check_labels, ignore=None):
        ops = _loss_operands(input, target, check_labels, ignore=ignore)
        state, out = _hybird_forward(ops, kind, gamma, weight_v, alpha, beta, smooth)
        _note_state(ops, state)
        ctx.save_for_backward(ops.x, ops.lab, state)
        ctx.meta = (ops.meta(), float(gamma), input.dtype, ignore)
        return out

    @staticmethod
    def backward(ctx, gout):
        x, lab, state = ctx.saved_tensors
        (st, lab_code, n, v, c), gamma, in_dtype, ignore = ctx.meta
        g, dz = _backward_prologue(gout, x)
        _hybird_backward(_view(x, st, lab, lab_code), n, v, c, gamma, state, g, dz, ignore)
        return _backward_epilogue(dz, in_dtype, 9)


class _FusedLoss(nn.Module):
    _kind = None

    def _ignore_for(self, input, target):
        """This module's ignore_label, checked against the C and the label dtype of the call."""
        ig = getattr(self, "ignore_label", None)
        if ig is None or input.dim() < 2:
            return None
        return _checked_softmax_ignore(ig, input.shape[1], target)

    def _call(self, input, target, gamma, weight_v, alpha, beta, smooth):
        return _FusedLossFn.apply(input, target, self._kind, gamma, weight_v, alpha, beta, smooth,
                                  getattr(self, "check_labels", _CHECK_LABELS), self._ignore_for(input, target))


class Dice(_FusedLoss):
    """Weighted mean Tversky/Dice *score* (a metric: higher is better)."""
    _kind = N.LOSS_DICE

    def __init__(self, weight_v=None, alpha=0.5, beta=0.5, smooth=1e-7, ignore_label=None):
        super().__init__()
        self.weight_v = weight_v
        self.alpha = alpha
        self.beta = beta
        self.smooth = smooth
        self.ignore_label = ignore_label

    def forward(self, input, target):
        return self._call(input, target, 2.0, self.weight_v, self.alpha, self.beta, self.smooth)


class DiceLoss(_FusedLoss):
    """sum_c w_c (1 - dice_c)."""
    _kind = N.LOSS_DICELOSS

    def __init__(self, weight_c=None, weight_v=None, alpha=0.5, beta=0.5, smooth=1e-7, ignore_label=None):
        super().__init__()
        self.weight_c = weight_c      # accepted, no effect (reference behaviour)
        self.weight_v = weight_v
        self.alpha = alpha
        self.beta = beta
        self.smooth = smooth
        self.ignore_label = ignore_label

    def forward(self, input, target):
        return self._call(input, target, 2.0, self.weight_v, self.alpha, self.beta, self.smooth)


class FocalLoss(_FusedLoss):
    """sum_c w_c * C * mean_v(-(1 - p_c)^gamma * onehot_c * log p_c)."""
    _kind = N.LOSS_FOCAL

    def __init__(self, gamma=2, weight_c=None, weight_v=None, ignore_label=None):
        super().__init__()
        self.gamma = gamma
        self.weight_c = weight_c      # accepted, no effect (reference behaviour)
        self.weight_v = weight_v
        self.ignore_label = ignore_label

    def forward(self, input, target):
        return self._call(input, target, self.gamma, self.weight_v, 0.5, 0.5, 1e-7)


class HybirdLoss(_FusedLoss):
    """sum_c w_c (1 - dice_c + focal_c): the training loss of the nb_train_* scripts."""
    _kind = N.LOSS_HYBIRD

    def __init__(self, gamma=2, weight_c=None, weight_v=None, alpha=0.5, beta=0.5, smooth=1e-7, ignore_label=None):
        super().__init__()
        self.weight_c = weight_c      # accepted, no effect (reference behaviour)
        self.weight_v = weight_v
        self.alpha = alpha
        self.beta = beta
        self.smooth = smooth
        self.gamma = gamma
        self.ignore_label = ignore_label

    def forward(self, input, target):
        return self._call(input, target, self.gamma, self.weight_v, self.alpha, self.beta, self.smooth)


def focal_loss(input, target, gamma=2, weight_c=None, weight_v=None):
    """Functional focal loss on flattened (N*V, C) scores and one-hot targets (reference signature)."""
    labels = target.argmax(dim=1) if target.dim() == 2 else target
    x = input.t().unsqueeze(0)          # (1, C, N*V): class axis second, voxels last
    return _FusedLossFn.apply(x, labels.reshape(1, -1), N.LOSS_FOCAL, gamma, weight_v, 0.5, 0.5, 1e-7,
                              _CHECK_LABELS)


# --------------------------------------------------------------------------- legacy names
class DiceCoef(Dice):
    """Pre-refactor name used by nb_train_KITS19.py / run_train.py: DiceCoef(weight=[...])."""

    def __init__(self, weight=None, alpha=0.5, beta=0.5, smooth=1e-7):
        super().__init__(weight_v=weight, alpha=alpha, beta=beta, smooth=smooth)


class FocalDiceCoefLoss(HybirdLoss):
    """Pre-refactor name used by nb_train_KITS19.py / run_train.py: FocalDiceCoefLoss(d_weight=[...])."""

    def __init__(self, d_weight=None, gamma=2, alpha=0.5, beta=0.5, smooth=1e-7):
        super().__init__(gamma=gamma, weight_v=d_weight, alpha=alpha, beta=beta, smooth=smooth)


# --------------------------------------------------------------------------- soft skeletons, soft-clDice
# The soft skeleton of Shit et al. (clDice, CVPR 2021) on (N, K, A, B, Z) volumes, Z fastest; nothing outside a volume takes
# part, nothing crosses between samples or classes:
#   E(x)[v] = min over v and its face neighbours, D(x)[v] = max over the 3x3x3 block, both clipped at the faces;
#   x_0 = x, x_{j+1} = E(x_j), d_j = relu(x_j - D(x_{j+1})), s_0 = d_0, s_j = s_{j-1} + relu(d_j - s_{j-1} d_j), S_k = s_k.
# (The paper's opening of x_j is D(E(x_j)) = D(x_{j+1}): one erosion and one dilation per iteration.)  A minimum or
# maximum hands its gradient to ONE voxel of its window, among equal candidates the one with the lowest linear index -
# every x_j with j >= 1 is made of plateaus of copied minima, so ties are the rule and the rule is part of the contract.
MAX_SKELETON_ITERATIONS = 64
_E_OFFSETS = ((-1, 0, 0), (0, -1, 0), (0, 0, -1), (0, 0, 0), (0, 0, 1), (0, 1, 0), (1, 0, 0))
_D_OFFSETS = tuple((da, db, dz) for da in (-1, 0, 1) for db in (-1, 0, 1) for dz in (-1, 0, 1))


def _window_extremum(x, offsets, fill, pick):
    """Host twin of E / D: the shifted copies stacked in ascending linear index, gathered at argmin / argmax (which
    return the first of equal extrema), so autograd follows the tie rule."""
    a, b, z = x.shape[-3:]
    xp = F.pad(x, (1, 1, 1, 1, 1, 1), value=fill)
    stack = torch.stack([xp[..., 1 + da:1 + da + a, 1 + db:1 + db + b, 1 + dz:1 + dz + z] for da, db, dz in offsets])
    return stack.gather(0, pick(stack.detach(), dim=0, keepdim=True))[0]


def soft_erode(x):
    """E on a host tensor (..., A, B, Z), in its own dtype."""
    return _window_extremum(x, _E_OFFSETS, float("inf"), torch.argmin)


def soft_dilate(x):
    """D on a host tensor (..., A, B, Z), in its own dtype."""
    return _window_extremum(x, _D_OFFSETS, float("-inf"), torch.argmax)


def _check_iterations(iterations):
    k = int(iterations)
    if k < 0 or k > MAX_SKELETON_ITERATIONS:
        raise N.Ru3dError("soft skeleton: iterations = %d (0 .. %d)" % (k, MAX_SKELETON_ITERATIONS))
    return k


def _soft_skeleton_host(x, k):
    xj, s = x, None
    for _ in range(k + 1):
        xn = soft_erode(xj)
        d = torch.relu(xj - soft_dilate(xn))
        s = d if s is None else s + torch.relu(d - s * d)
        xj = xn
    return s


def _skeleton_buffers(k, plane, dev):
    return (torch.empty((k + 1, plane), dtype=torch.float32, device=dev),
            torch.empty((k + 1, plane), dtype=torch.float32, device=dev),
            torch.empty((k + 1, plane), dtype=torch.uint8, device=dev),
            torch.empty((k + 1, plane), dtype=torch.uint8, device=dev))


class _SoftSkeletonFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, prob, k):
        N.require_device(prob, "soft_skeleton input")
        x = prob.detach().float().contiguous()
        n, kk, a, b, z = x.shape
        dev = x.device
        delta, s, emin, dmax = _skeleton_buffers(k, x.numel(), dev)
        ws = N.workspace(N.lib.ru3d_cldice_workspace_bytes(n * kk, a, b, z, k), dev)
        check(N.lib.ru3d_soft_skeleton_fwd(ptr(x), n * kk, a, b, z, k, ptr(delta), ptr(s), ptr(emin), ptr(dmax), ptr(ws),
                                           ws.numel(), stream()), "soft_skeleton_fwd")
        ctx.save_for_backward(delta, s, emin, dmax)
        ctx.meta = (tuple(x.shape), k, prob.dtype)
        return s[k].clone().view(x.shape)   # a copy: the caller may edit it in place, the saved planes stay intact

    @staticmethod
    def backward(ctx, gout):
        delta, s, emin, dmax = ctx.saved_tensors
        (n, kk, a, b, z), k, in_dtype = ctx.meta
        dev = delta.device
        g = gout.detach().to(device=dev, dtype=torch.float32).contiguous()
        N.note_device(dev)
        gx = torch.empty((n, kk, a, b, z), dtype=torch.float32, device=dev)
        ws = N.workspace(N.lib.ru3d_cldice_workspace_bytes(n * kk, a, b, z, k), dev)
        check(N.lib.ru3d_soft_skeleton_bwd(ptr(g), n * kk, a, b, z, k, ptr(delta), ptr(s), ptr(emin), ptr(dmax), ptr(gx),
                                           ptr(ws), ws.numel(), stream()), "soft_skeleton_bwd")
        return (gx if in_dtype == torch.float32 else gx.to(in_dtype)), None


def soft_skeleton(prob, iterations=3):
    """S_k of (N, K, A, B, Z) probabilities, differentiable.  HIP tensors go through the kernels and come back in
    float32; host tensors go through the torch twin above - the definition written down - in the dtype they have."""
    if prob.dim() != 5:
        raise N.Ru3dError("soft_skeleton: input must be (N, K, A, B, Z) - three spatial dimensions - not %s"
                          % (tuple(prob.shape),))
    k = _check_iterations(iterations)
    if prob.is_cuda:
        return _SoftSkeletonFn.apply(prob, k)
    return _soft_skeleton_host(prob, k)


def _selected_classes(what, classes, c):
    """The class selection of clDice and of the boundary loss (`what` names the loss): default 1 .. C-1."""
    cls = tuple(range(1, c)) if classes is None else tuple(int(q) for q in classes)
    if not cls or len(set(cls)) != len(cls) or min(cls) < 0 or max(cls) >= c:
        raise N.Ru3dError("%s: classes %s must be distinct class numbers of 0 .. %d" % (what, cls, c - 1))
    return cls


def _class_array(cls):
    """A class selection as the int array the ABI takes."""
    return N.ctypes.cast((N.ctypes.c_int * len(cls))(*cls), N.ctypes.c_void_p)


def _volume_shape_check(what, input):
    if input.dim() != 5:
        raise N.Ru3dError("%s: input must be (N, C, A, B, Z) - three spatial dimensions - not %s"
                          % (what, tuple(input.shape)))
    if input.shape[1] < 2:
        raise N.Ru3dError("%s: C == 1 is not supported (softmax over at least two classes)" % what)


def _soft_cldice_host(input, target, k, classes, weight_v, smooth):
    """The definition on host tensors, in the logits' dtype (what the device path is tested against)."""
    c = input.shape[1]
    cls = _selected_classes("clDice", classes, c)
    if weight_v is not None and len(weight_v) != c:
        raise RuntimeError("weight_v has %d entries for %d classes" % (len(weight_v), c))
    w = torch.tensor([1.0 if weight_v is None else float(weight_v[q]) for q in cls], dtype=input.dtype)
    w = w / w.abs().sum().clamp_min(1e-12)
    p = torch.softmax(input, dim=1)[:, list(cls)]
    g = F.one_hot(target.long(), num_classes=c).movedim(-1, 1)[:, list(cls)].to(input.dtype)
    sp, sg = _soft_skeleton_host(p, k), _soft_skeleton_host(g, k)
    dims = (0, 2, 3, 4)
    tprec = ((sp * g).sum(dims) + smooth) / (sp.sum(dims) + smooth)
    tsens = ((sg * p).sum(dims) + smooth) / (sg.sum(dims) + smooth)
    return (w * (1 - 2 * tprec * tsens / (tprec + tsens))).sum()


class _ClDiceFn(torch.autograd.Function):
    """(1 - cl_weight) Hybird + cl_weight clDice in one node (hyb = (gamma, weight_v, alpha, beta, smooth)), or the
    clDice term alone (hyb None): the clDice backward adds into the gradient the Hybird backward wrote."""

    @staticmethod
    def forward(ctx, input, target, hyb, cl_weight, k, classes, weight_v, smooth, check_labels):
        _volume_shape_check("clDice", input)
        ops = _loss_operands(input, target, check_labels)
        cls = _selected_classes("clDice", classes, ops.c)
        dev = ops.x.device
        n, vol, nsel = ops.n, tuple(ops.x.shape[2:]), len(cls)
        lam = float(cl_weight)
        state_h = None
        if hyb is not None:
            state_h, out_h = _hybird_forward(ops, N.LOSS_HYBIRD, *hyb)
        delta, s, emin, dmax = _skeleton_buffers(k, n * nsel * ops.v, dev)
        skel_g = torch.empty(n * nsel * ops.v, dtype=torch.float32, device=dev)
        state_c, out_c, ws, wv = _forward_scaffold(dev, N.lib.ru3d_cldice_state_bytes(),
                                                   N.lib.ru3d_cldice_workspace_bytes(n * nsel, *vol, k), weight_v, ops.c,
                                                   verdict=hyb is None)
        carr = _class_array(cls)
        check(N.lib.ru3d_cldice_fwd(*ops.view, n, *vol, ops.c, carr, nsel, k, wv,
                                    float(smooth), ptr(delta), ptr(s), ptr(emin), ptr(dmax), ptr(skel_g), ptr(state_c),
                                    ptr(out_c), ptr(ws), ws.numel(), stream()), "cldice_fwd")
        _note_state(ops, state_h, state_c)
        saved = [ops.x, ops.lab, delta, s, emin, dmax, skel_g, state_c]
        if state_h is not None:
            saved.append(state_h)
        ctx.save_for_backward(*saved)
        ctx.meta = (ops.meta(), carr, nsel, k, lam, None if hyb is None else float(hyb[0]), input.dtype)
        if state_h is None:
            return out_c
        return out_h * (1.0 - lam) + out_c * lam

    @staticmethod
    def backward(ctx, gout):
        x, lab, delta, s, emin, dmax, skel_g, state_c = ctx.saved_tensors[:8]
        (st, lab_code, n, v, c), carr, nsel, k, lam, gamma, in_dtype = ctx.meta
        view = _view(x, st, lab, lab_code)
        g, dz = _backward_prologue(gout, x)
        scale, accumulate = 1.0, 0
        if gamma is not None:
            _hybird_backward(view, n, v, c, gamma, ctx.saved_tensors[8], g * (1.0 - lam), dz)
            scale, accumulate = lam, 1
        vol = tuple(x.shape[2:])
        ws = N.workspace(N.lib.ru3d_cldice_workspace_bytes(n * nsel, *vol, k), x.device)
        check(N.lib.ru3d_cldice_bwd(*view, n, *vol, c, carr, nsel, k, ptr(delta),
                                    ptr(s), ptr(emin), ptr(dmax), ptr(skel_g), ptr(state_c), ptr(g), scale, accumulate,
                                    ptr(dz), ptr(ws), ws.numel(), stream()), "cldice_bwd")
        return _backward_epilogue(dz, in_dtype, 8)


class SoftClDiceLoss(_FusedLoss):
    """sum_{c in classes} w_c (1 - clDice_c), clDice_c the harmonic mean of
    Tprec_c = (sum S_k(P_c) G_c + smooth) / (sum S_k(P_c) + smooth) and
    Tsens_c = (sum S_k(G_c) P_c + smooth) / (sum S_k(G_c) + smooth), P = softmax(logits), G = one-hot(labels), sums over
    the batch's samples and voxels jointly; w = weight_v restricted to `classes` (default 1 .. C-1) over the sum of
    its absolute values.  Host tensors take the torch twin of the definition."""

    def __init__(self, iterations=3, weight_v=None, classes=None, smooth=1.0):
        super().__init__()
        self.iterations = _check_iterations(iterations)
        self.weight_v = weight_v
        self.classes = classes
        self.smooth = smooth

    def forward(self, input, target):
        if not input.is_cuda:
            _volume_shape_check("clDice", input)
            return _soft_cldice_host(input, target, self.iterations, self.classes, self.weight_v, self.smooth)
        return _ClDiceFn.apply(input, target, None, 1.0, self.iterations, self.classes, self.weight_v, self.smooth,
                               getattr(self, "check_labels", _CHECK_LABELS))


class HybirdClDiceLoss(_FusedLoss):
    """(1 - cl_weight) HybirdLoss(gamma, weight_c, weight_v, alpha, beta, smooth)
    + cl_weight SoftClDiceLoss(iterations, weight_v, classes, cl_smooth).  cl_weight == 0 is HybirdLoss itself: no
    clDice kernel is launched; cl_weight == 1 is the clDice term alone: no Hybird kernel is launched.  Device tensors
    only (host tensors raise, as with the other fused losses; SoftClDiceLoss has the host twin)."""
    _kind = N.LOSS_HYBIRD

    def __init__(self, cl_weight=0.5, iterations=3, classes=None, cl_smooth=1.0, gamma=2, weight_c=None, weight_v=None,
                 alpha=0.5, beta=0.5, smooth=1e-7):
        super().__init__()
        self.cl_weight = float(cl_weight)
        self.iterations = _check_iterations(iterations)
        self.classes = classes
        self.cl_smooth = cl_smooth
        self.gamma = gamma
        self.weight_c = weight_c      # accepted, no effect (reference behaviour)
        self.weight_v = weight_v
        self.alpha = alpha
        self.beta = beta
        self.smooth = smooth

    def forward(self, input, target):
        if self.cl_weight == 0.0:
            return self._call(input, target, self.gamma, self.weight_v, self.alpha, self.beta, self.smooth)
        hyb = None if self.cl_weight == 1.0 else (self.gamma, self.weight_v, self.alpha, self.beta, self.smooth)
        return _ClDiceFn.apply(input, target, hyb, self.cl_weight, self.iterations, self.classes, self.weight_v, self.cl_smooth,
                               getattr(self, "check_labels", _CHECK_LABELS))


# --------------------------------------------------------------------------- signed distance maps, boundary loss
# The boundary loss of Kervadec et al. (MIDL 2019): the mean of softmax probability x signed distance to the boundary of the
# ground truth.  The maps are made from the label patch as it is - after DeviceAugment cut, zoomed, warped and mirrored
# it - on the device, every step.  For sample n, class q, G = {label == q}:
#   v outside G: d2 = min over u in G of |v - u|^2, phi = +sqrt(d2);  v inside G: d2 = min over u outside G, phi = -(sqrt(d2) - 1)
#   (a foreground voxel on the boundary has phi = 0);  G empty or the whole volume of that sample: phi = 0, d2 = 0 there -
#   an absent class gives no loss and no gradient.  Distances are in voxels (unit spacing: there is no `sampling`
#   argument), nothing outside the patch exists, the patch faces are no boundary, a label outside [0, C) matches no class.
def _signed_squares_host(target, cls):
    """The written definition on a host tensor: int32 (N, K, A, B, Z), +d2 outside, -d2 inside, 0 where degenerate."""
    import numpy as np
    import scipy.ndimage as ndi
    lab = target.detach().cpu().numpy()
    out = np.zeros((lab.shape[0], len(cls)) + lab.shape[1:], dtype=np.int32)
    for n in range(lab.shape[0]):
        for k, q in enumerate(cls):
            g = lab[n] == q
            if not g.any() or g.all():
                continue
            # the transform is exact, so the square of the float64 distance it returns rounds to the integer it came from
            outside = np.rint(ndi.distance_transform_edt(~g) ** 2).astype(np.int32)
            inside = np.rint(ndi.distance_transform_edt(g) ** 2).astype(np.int32)
            out[n, k] = np.where(g, -inside, outside)
    return torch.from_numpy(out)


def _phi_of_squares(d2):
    """float32(sqrt(float64(d2))) outside, minus (that - 1) in float32 inside."""
    root = d2.abs().double().sqrt().float()
    return torch.where(d2 < 0, -(root - 1.0), root)


def signed_distance_map(target, num_classes, classes=None, squared=False):
    """(N, A, B, Z) integer labels -> (N, len(classes), A, B, Z) float32 signed distance maps phi as defined above, slot
    order following `classes` (default 1 .. num_classes - 1); squared=True gives the int32 signed squares instead: +d2
    outside, -d2 inside, 0 for a degenerate volume.  Unit spacing only: anisotropic `sampling` is not supported.  HIP
    tensors go through the kernels (all maps in one launch sequence, no host synchronisation); host tensors go through
    the numpy twin built on scipy.ndimage.distance_transform_edt - the definition written down."""
    if target.dim() != 4 or target.is_floating_point() or target.is_complex() or target.dtype == torch.bool:
        raise N.Ru3dError("signed_distance_map: target must be (N, A, B, Z) integer labels, not %s %s"
                          % (target.dtype, tuple(target.shape)))
    c = int(num_classes)
    if c < 2 or c > N.MAX_CLASSES:
        raise N.Ru3dError("signed_distance_map: %d classes (2 .. %d)" % (c, N.MAX_CLASSES))
    cls = _selected_classes("boundary", classes, c)
    if not target.is_cuda:
        d2 = _signed_squares_host(target, cls)
        return d2 if squared else _phi_of_squares(d2)
    N.require_device(target, "signed_distance_map target")
    lab, lab_code = _label_operand(target)
    n, a, b, z = lab.shape
    dev = lab.device
    nsel = len(cls)
    out = torch.empty((n, nsel, a, b, z), dtype=torch.int32 if squared else torch.float32, device=dev)
    need = N.lib.ru3d_boundary_workspace_bytes(n * nsel, a, b, z)
    ws = N.workspace(max(need, 1), dev)
    check(N.lib.ru3d_signed_distance(ptr(lab), lab_code, n, a, b, z, c, _class_array(cls), nsel,
                                     ptr(out) if squared else None, None if squared else ptr(out), ptr(ws),
                                     ws.numel() if need else 0, stream()), "signed_distance")
    return out


def _boundary_weights(weight_v, cls, c, dtype):
    if weight_v is not None and len(weight_v) != c:
        raise RuntimeError("weight_v has %d entries for %d classes" % (len(weight_v), c))
    w = torch.tensor([1.0 if weight_v is None else float(weight_v[q]) for q in cls], dtype=dtype)
    return w / w.abs().sum().clamp_min(1e-12)


def _boundary_host(input, target, classes, weight_v):
    """The definition on host tensors, in the logits' dtype (what the device path is tested against)."""
    c = input.shape[1]
    cls = _selected_classes("boundary", classes, c)
    w = _boundary_weights(weight_v, cls, c, input.dtype)
    if tuple(target.shape) != (input.shape[0],) + tuple(input.shape[2:]):
        raise N.Ru3dError("loss: target shape %s does not match input %s" % (tuple(target.shape), tuple(input.shape)))
    p = torch.softmax(input, dim=1)[:, list(cls)]
    phi = signed_distance_map(target.long(), c, cls).to(input.dtype)
    return (w * (p * phi).sum((0, 2, 3, 4))).sum() / (input.shape[0] * input[0, 0].numel())


class _BoundaryFn(torch.autograd.Function):
    """(1 - a) Hybird + a boundary in one node (hyb = (gamma, weight_v, alpha, beta, smooth), `a` a one-element float32
    device tensor read by device ops only, so a captured step follows it), or the boundary term alone (hyb None): the
    boundary backward adds into the gradient the Hybird backward wrote."""

    @staticmethod
    def forward(ctx, input, target, hyb, a, classes, weight_v, check_labels):
        _volume_shape_check("boundary", input)
        ops = _loss_operands(input, target, check_labels)
        cls = _selected_classes("boundary", classes, ops.c)
        dev = ops.x.device
        n, vol, nsel = ops.n, tuple(ops.x.shape[2:]), len(cls)
        state_h = None
        if hyb is not None:
            state_h, out_h = _hybird_forward(ops, N.LOSS_HYBIRD, *hyb)
        phi = torch.empty(n * nsel * ops.v, dtype=torch.float32, device=dev)
        need = N.lib.ru3d_boundary_workspace_bytes(n * nsel, *vol)
        state_b, out_b, ws, wv = _forward_scaffold(dev, N.lib.ru3d_boundary_state_bytes(), max(need, 1), weight_v, ops.c,
                                                   verdict=hyb is None)
        carr = _class_array(cls)
        check(N.lib.ru3d_boundary_fwd(*ops.view, n, *vol, ops.c, carr, nsel, wv, ptr(phi),
                                      ptr(state_b), ptr(out_b), ptr(ws), ws.numel() if need else 0, stream()),
              "boundary_fwd")
        _note_state(ops, state_h, state_b)
        saved = [ops.x, ops.lab, phi, state_b]
        if hyb is not None:
            a = a.detach().reshape(()).clone()        # the weight of THIS forward, whatever is set before the backward
            saved += [state_h, a]
        ctx.save_for_backward(*saved)
        ctx.meta = (ops.meta(), carr, nsel, None if hyb is None else float(hyb[0]), input.dtype)
        if hyb is None:
            return out_b
        return out_h * (1.0 - a) + out_b * a

    @staticmethod
    def backward(ctx, gout):
        x, lab, phi, state_b = ctx.saved_tensors[:4]
        (st, lab_code, n, v, c), carr, nsel, gamma, in_dtype = ctx.meta
        g, dz = _backward_prologue(gout, x)
        accumulate = 0
        if gamma is not None:
            state_h, a = ctx.saved_tensors[4:6]
            _hybird_backward(_view(x, st, lab, lab_code), n, v, c, gamma, state_h, g * (1.0 - a), dz)
            g = g * a
            accumulate = 1
        check(N.lib.ru3d_boundary_bwd(ptr(x), *st, n, *x.shape[2:], c, carr, nsel, ptr(phi), ptr(state_b), ptr(g), 1.0,
                                      accumulate, ptr(dz), stream()), "boundary_bwd")
        return _backward_epilogue(dz, in_dtype, 6)


class BoundaryLoss(_FusedLoss):
    """sum_{c in classes} w_c / (N V) sum_n sum_v P_c[n, v] phi_c[n, v]: the boundary term alone, P = softmax(logits), phi the
    signed distance maps of the labels (signed_distance_map; unit spacing; a class absent from a sample, or filling it,
    contributes nothing there), w = weight_v restricted to `classes` (default 1 .. C-1) over the sum of its absolute
    values.  The term is not bounded below: it is meant to be mixed into a region loss (HybirdBoundaryLoss).  Host
    tensors take the torch twin of the definition."""

    def __init__(self, weight_v=None, classes=None):
        super().__init__()
        self.weight_v = weight_v
        self.classes = classes

    def forward(self, input, target):
        if not input.is_cuda:
            _volume_shape_check("boundary", input)
            return _boundary_host(input, target, self.classes, self.weight_v)
        return _BoundaryFn.apply(input, target, None, None, self.classes, self.weight_v,
                                 getattr(self, "check_labels", _CHECK_LABELS))


class HybirdBoundaryLoss(_FusedLoss):
    """(1 - a) HybirdLoss(gamma, weight_c, weight_v, alpha, beta, smooth) + a BoundaryLoss(weight_v, classes), one autograd
    node.  `a` lives in a registered one-element float32 buffer and enters through device ops only, so a captured step
    (graph.GraphedTrainStep) follows it: set_boundary_weight(value) writes the buffer in place, stream-ordered, and the
    next replay uses the new value without a recapture - Kervadec's schedule raises it every epoch.  `boundary_weight`
    is the last value set, kept on the host (no read-back).  Both terms are always launched, whatever `a` is.  Device
    tensors only (host tensors raise, as with the other fused losses; BoundaryLoss has the host twin)."""
    _kind = N.LOSS_HYBIRD

    def __init__(self, boundary_weight=0.01, classes=None, gamma=2, weight_c=None, weight_v=None, alpha=0.5, beta=0.5,
                 smooth=1e-7):
        super().__init__()
        self._boundary_weight = float(boundary_weight)
        self.register_buffer("boundary_weight_buffer", torch.full((1,), self._boundary_weight, dtype=torch.float32))
        self.classes = classes
        self.gamma = gamma
        self.weight_c = weight_c      # accepted, no effect (reference behaviour)
        self.weight_v = weight_v
        self.alpha = alpha
        self.beta = beta
        self.smooth = smooth

    @property
    def boundary_weight(self):
        return self._boundary_weight

    def set_boundary_weight(self, value):
        """Write the weight into the device buffer in place (a fill on the current stream: ordered in front of the next
        step or replay, no synchronisation, no recapture)."""
        self._boundary_weight = float(value)
        self.boundary_weight_buffer.fill_(self._boundary_weight)

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)
        saved = state_dict.get(prefix + "boundary_weight_buffer")
        if saved is not None and saved.numel() == 1:
            self._boundary_weight = float(saved)      # the checkpoint's tensor, not the device buffer

    def forward(self, input, target):
        N.require_device(input, "loss input")
        if self.boundary_weight_buffer.device != input.device:
            # first call (an eager one: a captured step is warmed up first): the buffer follows the logits
            self.boundary_weight_buffer = self.boundary_weight_buffer.to(input.device)
        hyb = (self.gamma, self.weight_v, self.alpha, self.beta, self.smooth)
        return _BoundaryFn.apply(input, target, hyb, self.boundary_weight_buffer, self.classes, self.weight_v,
                                 getattr(self, "check_labels", _CHECK_LABELS))


# --------------------------------------------------------------------------- deep supervision
# nnU-Net's deep supervision: the network returns one logits tensor per supervised decoder level (network.Unet(...,
# deep_supervision=L), training mode), finest first; level l is judged against the labels at its own resolution and the
# total is sum_l w_l loss_l.  A level never gets a label tensor of its own: voxel (a, b, c) of level l has the label
# target[a * 2**l, b * 2**l, c * 2**l] - the strided view downsample_labels returns, with the extents ceil(full / 2**l).
# Where 2**l divides the extents this is F.interpolate(mode='nearest') of the labels to the level's extents; on an axis
# it does not divide, it is that of the labels padded to a multiple of 2**l (F.interpolate itself would step by
# full / ceil(full / 2**l) there).
def deep_supervision_weights(levels):
    """[2**-l for l in range(levels)] over their sum: the weights halve per level and add up to 1 (the nnU-Net rule over
    the levels in use)."""
    levels = int(levels)
    if levels < 1 or levels > N.DS_MAX_LEVELS:
        raise ValueError("deep supervision: %d levels (1 .. %d)" % (levels, N.DS_MAX_LEVELS))
    raw = [2.0 ** -l for l in range(levels)]
    total = sum(raw)
    return [r / total for r in raw]


def downsample_labels(target, level):
    """The labels level `level` of a deep-supervision loss sees: the view target[:, ::2**level, ::2**level, ...] of an
    (N, d1, ..., dn) label tensor (no copy; extents ceil(d / 2**level)).  Host and HIP tensors."""
    level = int(level)
    if level < 0:
        raise ValueError("downsample_labels: level %d" % level)
    step = 1 << level
    return target[(slice(None),) + (slice(None, None, step),) * (target.dim() - 1)]


def main_output(y):
    """The full-resolution logits of a model output: y[0] of the list a deep-supervision net returns in training mode, y
    itself otherwise."""
    return y[0] if isinstance(y, (list, tuple)) else y


def _counted_operands(z, t, c, ignore_label):
    """What the host twins do to (n, C, V) logits and (n, V) labels under an ignore label: the checked label, the mask of
    the counted voxels, and logits and labels with zeros at the ignored voxels (torch.where: whatever those logits hold,
    NaN included, reaches no value, and their gradient is exactly 0)."""
    ig = _checked_softmax_ignore(ignore_label, c, t)
    counted = t != ig
    return counted, torch.where(counted[:, None], z, torch.zeros((), dtype=z.dtype)), torch.where(counted, t, torch.zeros_like(t))


def _region_loss_host(kind, input, target, gamma, weight_v, alpha, beta, smooth, ignore_label=None):
    """HybirdLoss / DiceLoss / FocalLoss / Dice on host tensors with torch ops, in the logits' dtype: the formulas of the
    header comment of csrc/loss.hip (what the device path is tested against).  ignore_label: the section "ignore label"
    above - the sums run over the counted voxels and the focal mean divides by max(M, 1)."""
    n, c = input.shape[0], input.shape[1]
    if tuple(target.shape) != (n,) + tuple(input.shape[2:]):
        raise N.Ru3dError("loss: target shape %s does not match input %s" % (tuple(target.shape), tuple(input.shape)))
    if weight_v is not None and len(weight_v) != c:
        raise RuntimeError("weight_v has %d entries for %d classes" % (len(weight_v), c))
    z = input.reshape(n, c, -1)
    t = target.long().reshape(n, -1)
    counted = None
    if ignore_label is not None:
        counted, z, t = _counted_operands(z, target.reshape(n, -1), c, ignore_label)
        t = t.long()
    if t.numel() and (int(t.max()) >= c or int(t.min()) < 0):
        raise RuntimeError(_BAD_LABELS)
    logp = torch.log_softmax(z, dim=1) if c > 1 else F.logsigmoid(z)
    p = logp.exp()
    g = F.one_hot(t, num_classes=c).movedim(-1, 1).to(z.dtype)
    voxels = n * z.shape[2]
    if counted is not None:
        cm = counted[:, None].to(z.dtype)
        g, p = g * cm, p * cm       # p is used in the sums only
        voxels = max(int(counted.sum()), 1)
    w = torch.tensor([1.0] * c if weight_v is None else [float(a) for a in weight_v], dtype=z.dtype)
    w = w / w.abs().sum().clamp_min(1e-12)
    term = torch.zeros(c, dtype=z.dtype)
    if kind != N.LOSS_FOCAL:
        tp, sp, sg = (p * g).sum((0, 2)), p.sum((0, 2)), g.sum((0, 2))
        d = (tp + smooth) / (tp + alpha * (sg - tp) + beta * (sp - tp) + smooth)
        term = term + (d if kind == N.LOSS_DICE else 1.0 - d)
    if kind in (N.LOSS_HYBIRD, N.LOSS_FOCAL):
        # only the target class of a voxel contributes: gathered, so that log p = -inf of another class never meets a 0
        lt = logp.gather(1, t[:, None]) if c > 1 else logp
        per_voxel = -((1.0 - lt.exp()) ** gamma) * lt if gamma != 0 else -lt
        term = term + (g * per_voxel).sum((0, 2)) * c / voxels
    return (w * term).sum()


def _ds_levels(outputs, target):
    """Checks shared by the two routes: a list of (N, C, d, h, w) logits, finest first, level l with the extents
    ceil(full / 2**l), and (N, D, H, W) labels of level 0's extents."""
    if torch.is_tensor(outputs):
        outputs = [outputs]
    outputs = list(outputs)
    if not 1 <= len(outputs) <= N.DS_MAX_LEVELS:
        raise N.Ru3dError("deep supervision: %d outputs (1 .. %d)" % (len(outputs), N.DS_MAX_LEVELS))
    x0 = outputs[0]
    if x0.dim() != 5:
        raise N.Ru3dError("deep supervision: outputs must be (N, C, D, H, W) - three spatial dimensions - not %s"
                          % (tuple(x0.shape),))
    n, c = x0.shape[0], x0.shape[1]
    full = tuple(x0.shape[2:])
    if tuple(target.shape) != (n,) + full:
        raise N.Ru3dError("loss: target shape %s does not match input %s" % (tuple(target.shape), tuple(x0.shape)))
    for l, x in enumerate(outputs):
        want = (n, c) + tuple(-(-s // (1 << l)) for s in full)
        if tuple(x.shape) != want:
            raise N.Ru3dError("deep supervision: output %d has shape %s, level %d of %s is %s"
                              % (l, tuple(x.shape), l, tuple(x0.shape), want))
        if x.device != x0.device:
            raise N.Ru3dError("deep supervision: outputs on %s and %s" % (x0.device, x.device))
    return outputs


class _DeepSupFn(torch.autograd.Function):
    """All levels in one node: ru3d_ds_loss_fwd (one sums launch + one finalize) and ru3d_ds_loss_bwd (one launch), one
    gradient per listed logits tensor.  block: the criterion's persistent float32 block (weights | level losses | total)."""

    @staticmethod
    def forward(ctx, target, hyper, block, check_labels, *outputs):
        kind, gamma, weight_v, alpha, beta, smooth, ignore = hyper
        ops = _loss_operands(outputs, target, check_labels, ignore=ignore)
        table = (N.DsLevel * len(outputs))()
        for l, (x, st) in enumerate(zip(ops.x, ops.st)):
            table[l] = N.DsLevel(x.data_ptr(), *st, *x.shape[2:], l)
        n, c, full = ops.n, ops.c, tuple(outputs[0].shape[2:])
        state, out, ws, wv = _forward_scaffold(ops.lab.device, N.lib.ru3d_ds_state_bytes(),
                                               N.lib.ru3d_ds_loss_workspace_bytes(table, len(outputs), n), weight_v, c)
        if ignore is None:
            check(N.lib.ru3d_ds_loss_fwd(table, len(outputs), ptr(ops.lab), ops.lab_code, n, *full, c, kind, float(gamma),
                                         wv, float(alpha), float(beta), float(smooth), ptr(block), ptr(state), ptr(out),
                                         ptr(ws), ws.numel(), stream()), "ds_loss_fwd")
        else:
            check(N.lib.ru3d_ds_loss_ignore_fwd(table, len(outputs), ptr(ops.lab), ops.lab_code, n, *full, c,
                                                *_ignore_args(ignore), kind, float(gamma), wv, float(alpha), float(beta),
                                                float(smooth), ptr(block), ptr(state), ptr(out), ptr(ws), ws.numel(),
                                                stream()), "ds_loss_fwd")
        _note_state(ops, state, offset=_DS_BAD_OFF[0])
        ctx.save_for_backward(ops.lab, state, *ops.x)
        ctx.meta = (table, ops.lab_code, n, full, c, float(gamma), [x.dtype for x in outputs], ignore)
        return out

    @staticmethod
    def backward(ctx, gout):
        lab, state = ctx.saved_tensors[:2]
        xs = ctx.saved_tensors[2:]
        table, lab_code, n, full, c, gamma, in_dtypes, ignore = ctx.meta
        g, dzs = _upstream(gout, lab.device), [_empty_grad(x) for x in xs]
        dptr = (N.ctypes.c_void_p * len(dzs))(*[dz.data_ptr() for dz in dzs])
        if ignore is None:
            check(N.lib.ru3d_ds_loss_bwd(table, dptr, len(xs), ptr(lab), lab_code, n, *full, c, gamma, ptr(state), ptr(g),
                                         stream()), "ds_loss_bwd")
        else:
            check(N.lib.ru3d_ds_loss_ignore_bwd(table, dptr, len(xs), ptr(lab), lab_code, n, *full, c,
                                                *_ignore_args(ignore), gamma, ptr(state), ptr(g), stream()), "ds_loss_bwd")
        return (None, None, None, None) + tuple(_backward_epilogue(dz, dt) for dz, dt in zip(dzs, in_dtypes))


_DS_BAD_OFF = [int(N.lib.ru3d_ds_state_bad_labels_offset())]
assert _DS_BAD_OFF[0] >= _BAD_OFF[0]


class DeepSupervisionLoss(_FusedLoss):
    """sum_l w_l base(outputs[l], downsample_labels(target, l)) over the list a deep-supervision net returns in training
    mode (finest first; level l has the extents ceil(full / 2**l)), against the full-resolution labels.  `base` is a
    HybirdLoss, DiceLoss or FocalLoss instance whose hyper-parameters (gamma, weight_v, alpha, beta, smooth, ignore_label)
    are taken over when this module is built; with an ignore label a level's voxel is ignored iff the label it reads is
    the ignore label, and every level divides its focal sum by its own max(M_l, 1).  weights: one per level (default deep_supervision_weights(len(outputs))).  A single
    tensor instead of a list is one level with weight 1 - the plain base loss - so the same criterion object serves
    validation in eval mode.

    HIP tensors: all levels in one forward launch pair and one backward launch (csrc/deepsup.hip), no label copies; the
    level weights are read from device memory, so set_weights() between the replays of a captured step
    (graph.GraphedTrainStep) takes effect without a recapture.  Host tensors: the torch twin of the definition."""

    def __init__(self, base, weights=None):
        super().__init__()
        if not isinstance(base, (HybirdLoss, DiceLoss, FocalLoss)):
            raise TypeError("DeepSupervisionLoss wraps a HybirdLoss, DiceLoss or FocalLoss instance, not %s"
                            % type(base).__name__)
        self._kind = base._kind
        self.gamma = getattr(base, "gamma", 2.0)
        self.weight_v = base.weight_v
        self.alpha = getattr(base, "alpha", 0.5)
        self.beta = getattr(base, "beta", 0.5)
        self.smooth = getattr(base, "smooth", 1e-7)
        self.ignore_label = getattr(base, "ignore_label", None)
        if hasattr(base, "check_labels"):
            self.check_labels = base.check_labels
        self._weights = None
        self._blocks = {}         # (device, levels) -> float32 block [weights 0..7 | level losses 8..15 | total 16]
        self._last = None         # (block, levels) of the last call
        if weights is not None:
            self._weights = self._checked(weights)

    @staticmethod
    def _checked(ws):
        ws = [float(w) for w in ws]
        if not 1 <= len(ws) <= N.DS_MAX_LEVELS:
            raise ValueError("deep supervision: %d weights (1 .. %d)" % (len(ws), N.DS_MAX_LEVELS))
        return ws

    @property
    def weights(self):
        """The weights last set (host copy; None: the default rule for however many levels a call brings)."""
        return None if self._weights is None else list(self._weights)

    def _weights_for(self, levels):
        if levels == 1:
            return [1.0]
        if self._weights is None:
            return deep_supervision_weights(levels)
        if len(self._weights) != levels:
            raise ValueError("deep supervision: %d outputs but %d weights" % (levels, len(self._weights)))
        return self._weights

    @staticmethod
    def _write(block, ws):
        # fills with host scalars: stream-ordered, no synchronisation, legal while a step is being captured
        for l, w in enumerate(ws):
            block[l:l + 1].fill_(w)

    def _block(self, device, levels):
        key = (device, levels)
        block = self._blocks.get(key)
        if block is None:
            block = self._blocks[key] = torch.zeros(2 * N.DS_MAX_LEVELS + 1, dtype=torch.float32, device=device)
            self._write(block, self._weights_for(levels))
        return block

    def set_weights(self, ws):
        """New level weights, written in place into the device block(s) the kernels read (fills on the current stream:
        ordered in front of the next call or replay, no synchronisation, no recapture, no new allocation)."""
        self._weights = self._checked(ws)
        for (device, levels), block in self._blocks.items():
            if levels == len(self._weights) and levels > 1:
                self._write(block, self._weights)

    @property
    def last_level_losses(self):
        """float32 [L]: the levels' un-weighted losses of the last call, on the logits' device.  A view of this module's
        persistent block, rewritten by the next call (or replay): .clone() it to keep it."""
        if self._last is None:
            return None
        block, levels = self._last
        return block[N.DS_MAX_LEVELS:N.DS_MAX_LEVELS + levels]

    def forward(self, outputs, target):
        outputs = _ds_levels(outputs, target)
        levels = len(outputs)
        if not outputs[0].is_cuda:
            ws = self._weights_for(levels)
            per = [_region_loss_host(self._kind, x, downsample_labels(target, l), self.gamma, self.weight_v, self.alpha,
                                     self.beta, self.smooth, self.ignore_label) for l, x in enumerate(outputs)]
            self._last = (torch.cat([torch.zeros(N.DS_MAX_LEVELS)] + [v.detach().float().reshape(1) for v in per]), levels)
            return sum(w * v for w, v in zip(ws, per))
        block = self._block(outputs[0].device, levels)
        self._last = (block, levels)
        hyper = (self._kind, self.gamma, self.weight_v, self.alpha, self.beta, self.smooth,
                 self._ignore_for(outputs[0], target))
        return _DeepSupFn.apply(target, hyper, block, getattr(self, "check_labels", _CHECK_LABELS), *outputs)


# --------------------------------------------------------------------------- overlapping label groups
# One sigmoid channel per GROUP of label values (the KiTS / BraTS recipe of nnU-Net).  groups = ((1, 2), (2,)) reads
# "whole kidney, tumour": a voxel labelled 2 is a target of both channels.  member[t] has bit k set iff label value t is in
# group k; the kernels read the target of channel k as that bit of member[label], so no multi-hot tensor exists.  Over the
# counted voxels (those not carrying ignore_label; M of them, max(M, 1) where it divides), p = sigmoid(z_k), g the target:
#   dice_k  = (tp + s) / (tp + alpha (sg - tp) + beta (sp - tp) + s),  tp = sum p g, sp = sum p, sg = sum g
#   focal_k = (1 / M) sum [ (1-p)^gamma g softplus(-z) + p^gamma (1-g) softplus(z) ]          (gamma 0: binary CE)
#   w = weight_v / sum|weight_v|;  GroupHybirdLoss = sum_k w_k (1 - dice_k + focal_k), GroupDiceLoss = sum w (1 - dice),
#   GroupFocalLoss = sum w focal, GroupDice = sum w dice.
MAX_GROUPS = N.MAX_CLASSES
MAX_GROUP_LABELS = 32


def _checked_groups(groups, num_labels=None):
    """(tuple of K tuples of ints, T) of a `groups` argument, or ValueError."""
    try:
        gs = tuple(tuple(int(t) for t in g) for g in groups)
    except TypeError:
        raise ValueError("groups must be a sequence of sequences of label values, got %r" % (groups,))
    if not 1 <= len(gs) <= MAX_GROUPS:
        raise ValueError("groups: %d groups (1 .. %d)" % (len(gs), MAX_GROUPS))
    for k, g in enumerate(gs):
        if not g:
            raise ValueError("groups: group %d is empty" % k)
        if len(set(g)) != len(g):
            raise ValueError("groups: group %d repeats a label value: %s" % (k, g))
        if min(g) < 0:
            raise ValueError("groups: group %d holds a negative label value: %s" % (k, g))
    if len(set(frozenset(g) for g in gs)) != len(gs):
        raise ValueError("groups: two groups are equal as sets: %s" % (gs,))
    top = max(max(g) for g in gs)
    t = top + 1 if num_labels is None else int(num_labels)
    if t > MAX_GROUP_LABELS or t < 1:
        raise ValueError("groups: %d label values (1 .. %d)" % (t, MAX_GROUP_LABELS))
    if top >= t:
        raise ValueError("groups: label value %d lies outside [0, %d)" % (top, t))
    return gs, t


def group_table(groups, num_labels=None):
    """The membership table of `groups`: T = num_labels (default 1 + the largest value) bytes, bit k of byte t set iff
    label value t is in group k.  Checks the groups (1 .. 8 of them, values in [0, T), T <= 32, no empty group, no
    repeated value, no two groups equal as sets) with ValueError."""
    gs, t = _checked_groups(groups, num_labels)
    table = bytearray(t)
    for k, g in enumerate(gs):
        for v in g:
            table[v] |= 1 << k
    return bytes(table)


def _checked_ignore(ignore_label, t):
    if ignore_label is None:
        return None
    ig = int(ignore_label)
    if 0 <= ig < t:
        raise ValueError("ignore_label %d lies inside the label range [0, %d)" % (ig, t))
    return ig


def _group_loss_host(kind, input, target, table, ignore, gamma, weight_v, alpha, beta, smooth):
    """The definitions above on host tensors with torch ops, differentiable, in the logits' dtype: the twin the kernels
    are held to."""
    n, k = input.shape[0], input.shape[1]
    if tuple(target.shape) != (n,) + tuple(input.shape[2:]):
        raise N.Ru3dError("loss: target shape %s does not match input %s" % (tuple(target.shape), tuple(input.shape)))
    z = input.reshape(n, k, -1)
    t = target.long().reshape(n, 1, -1)
    counted = torch.ones_like(t, dtype=torch.bool) if ignore is None else t != ignore
    if t.numel() and bool((((t < 0) | (t >= len(table))) & counted).any()):
        raise RuntimeError(_BAD_LABELS)
    member = torch.tensor(list(table), dtype=torch.int64)
    bits = member[t.clamp(0, len(table) - 1)]
    g = ((bits >> torch.arange(k).view(1, k, 1)) & 1).to(z.dtype)
    c = counted.to(z.dtype)
    g = g * c
    p = torch.sigmoid(z)
    w = torch.tensor([1.0] * k if weight_v is None else [float(a) for a in weight_v], dtype=z.dtype)
    w = w / w.abs().sum().clamp_min(1e-12)
    term = torch.zeros(k, dtype=z.dtype)
    if kind != N.LOSS_FOCAL:
        tp, sp, sg = (p * g).sum((0, 2)), (p * c).sum((0, 2)), g.sum((0, 2))
        d = (tp + smooth) / (tp + alpha * (sg - tp) + beta * (sp - tp) + smooth)
        term = term + (d if kind == N.LOSS_DICE else 1.0 - d)
    if kind in (N.LOSS_HYBIRD, N.LOSS_FOCAL):
        pos, neg = F.softplus(-z), F.softplus(z)          # -log p, -log(1 - p), from the logit
        if gamma != 0:
            pos, neg = (1.0 - p) ** gamma * pos, p ** gamma * neg
        m = c.sum().clamp_min(1.0)
        term = term + ((g * pos + (c - g) * neg).sum((0, 2))) / m
    return (w * term).sum()


class _GroupLossFn(torch.autograd.Function):
    """Written out in full, not on the scaffolds the other five Functions share: on them its forward + backward cost the
    host about 0.008 ms more than before (profiles/loss_call_path_check.txt), and no cause was found.  It takes the
    operands as the plain tuple of _operand_parts."""

    @staticmethod
    def forward(ctx, input, target, kind, table, ignore, gamma, weight_v, alpha, beta, smooth, check_labels):
        k, t = input.shape[1], len(table)
        N.require_device(input, "loss input")
        if check_labels and target.numel():
            lab = target if ignore is None else target[target != ignore]
            if lab.numel() and (int(lab.max()) >= t or int(lab.min()) < 0):
                raise RuntimeError(_BAD_LABELS)
        x, lab, st, lab_code, n, _, v, _ = _operand_parts(input, target, False, False)
        raise_on_bad_labels()          # an earlier call's verdict, if it has landed (no wait)
        dev = x.device
        state = torch.empty(N.lib.ru3d_group_loss_state_bytes(), dtype=torch.uint8, device=dev)
        out = torch.empty((), dtype=torch.float32, device=dev)
        ws = N.workspace(N.lib.ru3d_group_loss_workspace_bytes(n, v, k), dev)
        wv = _weight_array(weight_v, k)
        group = (table, t, 0 if ignore is None else 1, 0 if ignore is None else ignore)
        check(N.lib.ru3d_group_loss_fwd(ptr(x), st[0], st[1], st[2], ptr(lab), lab_code, n, v, k, *group, kind,
                                        float(gamma), N.ctypes.cast(wv, N.ctypes.c_void_p) if wv is not None else None,
                                        float(alpha), float(beta), float(smooth), ptr(state), ptr(out), ptr(ws),
                                        ws.numel(), stream()), "group_loss_fwd")
        if not check_labels:
            _note_label_flag(state)
        ctx.save_for_backward(x, lab, state)
        ctx.meta = (st, lab_code, n, v, k, group, float(gamma), input.dtype)
        return out

    @staticmethod
    def backward(ctx, gout):
        x, lab, state = ctx.saved_tensors
        st, lab_code, n, v, k, group, gamma, in_dtype = ctx.meta
        g = gout.detach()
        if g.dtype != torch.float32 or g.device != x.device:
            g = g.to(device=x.device, dtype=torch.float32)
        g = g.reshape(1).contiguous()
        N.note_device(x.device)
        dz = torch.empty_like(x)   # preserve_format: same (dense) strides as the logits
        if dz.stride() != x.stride():
            dz = torch.empty_strided(x.shape, x.stride(), dtype=x.dtype, device=x.device)
        check(N.lib.ru3d_group_loss_bwd(ptr(x), st[0], st[1], st[2], ptr(lab), lab_code, n, v, k, *group, gamma,
                                        ptr(state), ptr(g), ptr(dz), N.F32, stream()), "group_loss_bwd")
        if in_dtype != torch.float32:
            dz = dz.to(in_dtype)
        return (dz,) + (None,) * 10


class _GroupLoss(_FusedLoss):
    """What the four group losses share: the checked groups, their table, and the route by the logits' device."""

    def _init_groups(self, groups, num_labels, ignore_label, weight_v):
        self.groups, self.num_labels = _checked_groups(groups, num_labels)
        self._table = group_table(self.groups, self.num_labels)
        self.ignore_label = _checked_ignore(ignore_label, self.num_labels)
        if weight_v is not None and len(weight_v) != len(self.groups):
            raise ValueError("weight_v has %d entries for %d groups" % (len(weight_v), len(self.groups)))
        self.weight_v = weight_v

    def _call(self, input, target, gamma, weight_v, alpha, beta, smooth):
        if input.dim() < 2 or input.shape[1] != len(self.groups):
            raise ValueError("%s: the logits have shape %s; %d groups need %d channels"
                             % (type(self).__name__, tuple(input.shape), len(self.groups), len(self.groups)))
        if not input.is_cuda:
            return _group_loss_host(self._kind, input, target, self._table, self.ignore_label, gamma, weight_v, alpha,
                                    beta, smooth)
        return _GroupLossFn.apply(input, target, self._kind, self._table, self.ignore_label, gamma, weight_v, alpha,
                                  beta, smooth, getattr(self, "check_labels", _CHECK_LABELS))


class GroupDice(_GroupLoss):
    """sum_k w_k dice_k over the label groups: a metric, higher is better."""
    _kind = N.LOSS_DICE

    def __init__(self, groups, num_labels=None, ignore_label=None, weight_v=None, alpha=0.5, beta=0.5, smooth=1e-7):
        super().__init__()
        self._init_groups(groups, num_labels, ignore_label, weight_v)
        self.alpha = alpha
        self.beta = beta
        self.smooth = smooth

    def forward(self, input, target):
        return self._call(input, target, 2.0, self.weight_v, self.alpha, self.beta, self.smooth)


class GroupDiceLoss(_GroupLoss):
    """sum_k w_k (1 - dice_k) over the label groups."""
    _kind = N.LOSS_DICELOSS

    def __init__(self, groups, num_labels=None, ignore_label=None, weight_v=None, alpha=0.5, beta=0.5, smooth=1e-7):
        super().__init__()
        self._init_groups(groups, num_labels, ignore_label, weight_v)
        self.alpha = alpha
        self.beta = beta
        self.smooth = smooth

    def forward(self, input, target):
        return self._call(input, target, 2.0, self.weight_v, self.alpha, self.beta, self.smooth)


class GroupFocalLoss(_GroupLoss):
    """sum_k w_k focal_k: the binary focal loss of every group channel (gamma = 0: binary cross-entropy)."""
    _kind = N.LOSS_FOCAL

    def __init__(self, groups, num_labels=None, ignore_label=None, weight_v=None, gamma=2):
        super().__init__()
        self._init_groups(groups, num_labels, ignore_label, weight_v)
        self.gamma = gamma

    def forward(self, input, target):
        return self._call(input, target, self.gamma, self.weight_v, 0.5, 0.5, 1e-7)


class GroupHybirdLoss(_GroupLoss):
    """sum_k w_k (1 - dice_k + focal_k) over the label groups: HybirdLoss for nested or overlapping structures.  The
    logits have one channel per group (network out_channels = len(groups)); targets stay the plain label map.  HIP
    tensors run the kernels of csrc/groups.hip, host tensors the torch twin of the definitions."""
    _kind = N.LOSS_HYBIRD

    def __init__(self, groups, num_labels=None, ignore_label=None, weight_v=None, gamma=2, alpha=0.5, beta=0.5,
                 smooth=1e-7):
        super().__init__()
        self._init_groups(groups, num_labels, ignore_label, weight_v)
        self.gamma = gamma
        self.alpha = alpha
        self.beta = beta
        self.smooth = smooth

    def forward(self, input, target):
        return self._call(input, target, self.gamma, self.weight_v, self.alpha, self.beta, self.smooth)


# --------------------------------------------------------------------------- top-k cross-entropy
# nnU-Net's TopKLoss and DC_and_topk_loss.  Over the M = N * V voxels of the batch, flattened as nnU-Net flattens them:
#   ce_v = -log softmax(z_v)[t_v],  K = max(1, int(M * k / 100)),  tau = the K-th largest ce,
#   G = #{ce > tau},  E = #{ce == tau},  topk = (sum_{ce > tau} ce + (K - G) * tau) / K   (= torch.topk(ce, K).values.mean())
#   d topk / d z_{v,c} = s_v (p_{v,c} - [c == t_v]) / K,  s_v = 1 if ce_v > tau, (K - G) / E if ce_v == tau, else 0.
# The voxels tied at the threshold share the remaining weight equally: the loss is deterministic and does not depend on
# the order of the voxels; it is torch.topk's gradient whenever E == 1.  The tie rule is part of the contract - ties at
# ce == 0 are real for saturated voxels.  k = 100 is the plain mean cross-entropy.
#   TopKLoss = topk,  HybirdTopKLoss = sum_c w_c (1 - dice_c) + ce_weight * topk with DiceLoss's w and Tversky dice_c.
def topk_count(voxels, k):
    """K of a batch of `voxels` voxels: max(1, int(voxels * k / 100))."""
    return max(1, int(voxels * k / 100))


def _checked_k(k):
    k = float(k)
    if not 0.0 < k <= 100.0:
        raise ValueError("top-k loss: k = %g percent lies outside (0, 100]" % k)
    return k


def _topk_checks(input, weight_v):
    if input.dim() < 2:
        raise N.Ru3dError("loss: input must be (N, C, d1, ..., dn)")
    c = input.shape[1]
    if c < 2:
        raise ValueError("top-k loss: C == 1 is not supported (softmax over at least two classes)")
    if weight_v is not None and len(weight_v) != c:
        raise ValueError("weight_v has %d entries for %d classes" % (len(weight_v), c))


def _topk_loss_host(input, target, k, with_dice=False, weight_v=None, alpha=0.5, beta=0.5, smooth=1e-7, ce_weight=1.0,
                    ignore_label=None):
    """The definitions above on host tensors with torch ops, differentiable, in the logits' dtype, the tie rule included:
    the twin the kernels are held to.  ignore_label: an ignored voxel has ce = 0 and is selected like any voxel whose
    cross-entropy is 0; K counts all voxels."""
    _topk_checks(input, weight_v)
    n, c = input.shape[0], input.shape[1]
    if tuple(target.shape) != (n,) + tuple(input.shape[2:]):
        raise N.Ru3dError("loss: target shape %s does not match input %s" % (tuple(target.shape), tuple(input.shape)))
    z = input.reshape(n, c, -1)
    t = target.long().reshape(n, -1)
    counted = None
    if ignore_label is not None:
        counted, z, t = _counted_operands(z, target.reshape(n, -1), c, ignore_label)
        t = t.long()
    if t.numel() and (int(t.max()) >= c or int(t.min()) < 0):
        raise RuntimeError(_BAD_LABELS)
    ce = -torch.log_softmax(z, dim=1).gather(1, t[:, None]).reshape(-1)
    if counted is not None:
        ce = torch.where(counted.reshape(-1), ce, torch.zeros((), dtype=ce.dtype))
    kk = topk_count(ce.numel(), _checked_k(k))
    held = ce.detach()
    tau = torch.topk(held, kk).values[-1]
    above, tied = held > tau, held == tau
    share = (kk - int(above.sum())) / int(tied.sum())
    s = above.to(ce.dtype) + tied.to(ce.dtype) * share
    value = (s * ce).sum() / kk * ce_weight
    if with_dice:
        value = value + _region_loss_host(N.LOSS_DICELOSS, input, target, 2.0, weight_v, alpha, beta, smooth,
                                          ignore_label)
    return value


class _TopKLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, input, target, kk, with_dice, weight_v, alpha, beta, smooth, ce_weight, check_labels, ignore=None):
        ops = _loss_operands(input, target, check_labels, ignore=ignore)
        n, v, c = ops.n, ops.v, ops.c
        state, out, ws, wv = _forward_scaffold(ops.x.device, N.lib.ru3d_topk_loss_state_bytes(),
                                               N.lib.ru3d_topk_loss_workspace_bytes(n, v, c), weight_v, c)
        # the backward compares these stored values with tau: a tensor of this call, not a slice of the shared workspace,
        # which other calls reuse between a forward and its backward
        ce = torch.empty(n * v, dtype=torch.float32, device=ops.x.device)
        if ignore is None:
            check(N.lib.ru3d_topk_loss_fwd(*ops.view, n, v, c, kk, int(with_dice), wv, float(alpha),
                                           float(beta), float(smooth), float(ce_weight), ptr(ce), ptr(state), ptr(out),
                                           ptr(ws), ws.numel(), stream()), "topk_loss_fwd")
        else:
            check(N.lib.ru3d_topk_loss_ignore_fwd(*ops.view, n, v, c, *_ignore_args(ignore), kk, int(with_dice), wv,
                                                  float(alpha), float(beta), float(smooth), float(ce_weight), ptr(ce),
                                                  ptr(state), ptr(out), ptr(ws), ws.numel(), stream()), "topk_loss_fwd")
        _note_state(ops, state)
        ctx.save_for_backward(ops.x, ops.lab, ce, state)
        ctx.meta = (ops.meta(), int(with_dice), input.dtype, ignore)
        return out

    @staticmethod
    def backward(ctx, gout):
        x, lab, ce, state = ctx.saved_tensors
        (st, lab_code, n, v, c), with_dice, in_dtype, ignore = ctx.meta
        g, dz = _backward_prologue(gout, x)
        if ignore is None:
            check(N.lib.ru3d_topk_loss_bwd(*_view(x, st, lab, lab_code), n, v, c, with_dice, ptr(ce), ptr(state),
                                           ptr(g), ptr(dz), N.F32, stream()), "topk_loss_bwd")
        else:
            check(N.lib.ru3d_topk_loss_ignore_bwd(*_view(x, st, lab, lab_code), n, v, c, *_ignore_args(ignore), with_dice,
                                                  ptr(ce), ptr(state), ptr(g), ptr(dz), N.F32, stream()), "topk_loss_bwd")
        return _backward_epilogue(dz, in_dtype, 10)


class _TopKLoss(_FusedLoss):
    """What the two top-k losses share: the checked k and the route by the logits' device."""
    _with_dice = False

    def _call_topk(self, input, target, weight_v, alpha, beta, smooth, ce_weight):
        _topk_checks(input, weight_v)
        ignore = self._ignore_for(input, target)
        if not input.is_cuda:
            return _topk_loss_host(input, target, self.k, self._with_dice, weight_v, alpha, beta, smooth, ce_weight,
                                   ignore)
        voxels = input.shape[0]
        for s in input.shape[2:]:
            voxels *= s
        return _TopKLossFn.apply(input, target, topk_count(voxels, self.k), self._with_dice, weight_v, alpha, beta,
                                 smooth, ce_weight, getattr(self, "check_labels", _CHECK_LABELS), ignore)


class TopKLoss(_TopKLoss):
    """The cross-entropy averaged over the hardest k percent of the batch's voxels (nnU-Net's TopKLoss, k = 10): the mean of
    the K = max(1, int(N * V * k / 100)) largest -log softmax(z_v)[t_v]; k = 100 is the plain mean cross-entropy.  Voxels
    tied at the threshold share the weight that is left equally (the section comment above).  k is fixed at construction,
    0 < k <= 100; K is a launch argument of a captured step (graph.GraphedTrainStep), so another k - or another batch
    shape - means a recapture.  C >= 2.  HIP tensors run the kernels of csrc/topk.hip (no sort, no host round trip
    between the forward and the backward), host tensors the torch twin of the definitions.  ignore_label (nnU-Net's
    ignore_index rule): an ignored voxel has ce = 0, takes part in the selection like any voxel whose cross-entropy is 0
    and gets a zero gradient; K stays relative to ALL N * V voxels - a K relative to the counted voxels would have to be
    computed on the device and is not implemented."""

    def __init__(self, k=10, ignore_label=None):
        super().__init__()
        self.k = _checked_k(k)
        self.ignore_label = ignore_label

    def forward(self, input, target):
        return self._call_topk(input, target, None, 0.5, 0.5, 1e-7, 1.0)


class HybirdTopKLoss(_TopKLoss):
    """sum_c w_c (1 - dice_c) + ce_weight * topk: DiceLoss(weight_v, alpha, beta, smooth) plus TopKLoss(k), nnU-Net's
    DC_and_topk_loss, in one forward pass over logits and labels and one backward pass.  k is fixed at construction,
    0 < k <= 100; K = max(1, int(N * V * k / 100)) is a launch argument of a captured step, so another k - or another
    batch shape - means a recapture.  C >= 2.  HIP tensors run the kernels of csrc/topk.hip, host tensors the torch twin.
    ignore_label: as TopKLoss's for the cross-entropy leg (K relative to all voxels; a K relative to the counted voxels
    is not implemented), and the Dice leg sums over the counted voxels only."""
    _with_dice = True

    def __init__(self, k=10, weight_v=None, alpha=0.5, beta=0.5, smooth=1e-7, ce_weight=1.0, ignore_label=None):
        super().__init__()
        self.ignore_label = ignore_label
        self.k = _checked_k(k)
        self.weight_v = weight_v
        self.alpha = alpha
        self.beta = beta
        self.smooth = smooth
        self.ce_weight = ce_weight

    def forward(self, input, target):
        return self._call_topk(input, target, self.weight_v, self.alpha, self.beta, self.smooth, self.ce_weight)
