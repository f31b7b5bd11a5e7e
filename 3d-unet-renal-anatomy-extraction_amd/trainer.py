"""Drop-in `trainer` module: host-side driver of the native training step.

Keeps the reference `Trainer` surface (reference trainer.py:415-634: constructor arguments,
`fit(num_epochs, save_dir, use_amp, opt_level)`, `batch_loop`, `save_checkpoint` / `load_checkpoint`
with the same checkpoint keys, `get_lr` / `set_lr` / `summary`, `Subset`) and the pre-refactor
spelling the oldest script uses (reference run_train.py:71-96: `Trainer(criterion=, tr_transform=,
vd_transform=)`, `fit(dataset, batch_size=, epochs=, ...)`, `save` / `load`).

What changes underneath:
  * `use_amp=True` selects 16-bit storage / fp32 accumulation of the native kernels: fp16 with dynamic loss
    scaling for the reference's opt_level 'O1' (apex patched fp16 convs in, trainer.py:538-542, and scaled the
    loss, :492-493), or bf16 without loss scaling for opt_level='bf16'.
  * per-step `.item()` calls are deferred: the loss/metric scalars stay on the device and are read
    back once per `sync_every` steps (default: every step, the reference's behaviour), so the GPU
    is not drained between kernels.  The NaN rule is the reference's: a NaN step is excluded from
    the epoch mean but its optimizer step has already been applied (trainer.py:496 vs 505-506).
  * one process per GPU: when torch.distributed is initialised, gradients are averaged across
    ranks by `parallel.GradSync` (bucketed RCCL all-reduce on a side stream, overlapped with the
    rest of backward) and each rank draws its own samples.
  * apex / torchsummary / tensorboard / nibabel are optional.
"""
import gc
import math
import os

import numpy as np
import torch
from torch.optim import lr_scheduler

try:
    from tqdm import tqdm
except Exception:  # pragma: no cover
    tqdm = None
try:
    from torch.utils.tensorboard import SummaryWriter
except Exception:
    SummaryWriter = None

from loss import dice  # noqa: F401  (re-exported like the reference: trainer.dice)
import loss as _loss_mod
from inference import predict_per_patch, predict_case  # noqa: F401  (reference trainer.py:17, 101)


class _NullBar:
    def __init__(self, *a, **k):
        pass

    def reset(self, total=None):
        pass

    def set_description(self, *a, **k):
        pass

    def set_postfix(self, *a, **k):
        pass

    def update(self, *a, **k):
        pass

    def close(self):
        pass


class Subset(torch.utils.data.Subset):
    """Index subset that applies a transform to each fetched case."""

    def __init__(self, dataset, indices, transform):
        super().__init__(dataset, indices)
        self.transform = transform

    def __getitem__(self, idx):
        case = self.dataset[self.indices[idx]]
        return self.transform(case) if self.transform else case

    def __getitems__(self, indices):
        # torch >= 2.0 loaders fetch batches through __getitems__, and the inherited one reads self.dataset directly:
        # the transform of the reference's class (trainer.py:403-412, written for the per-item protocol) would be skipped
        return [self[i] for i in indices]


def _dist_ready():
    return torch.distributed.is_available() and torch.distributed.is_initialized() \
        and torch.distributed.get_world_size() > 1


class _RankShardSampler(torch.utils.data.Sampler):
    """One process per GPU, one pass over the split per epoch: every epoch draws ONE permutation that is the same on all
    ranks (seed + epoch counter) and this rank takes every world-th case of it, wrapped so that all ranks take the same
    number of steps (the gradient exchange is collective).  The permutation changes with every __iter__, like the
    reference's `shuffle=True` loader (trainer.py:543-547)."""

    def __init__(self, n, rank, world, shuffle, seed, epoch=0):
        self.n, self.rank, self.world, self.shuffle, self.seed, self.epoch = n, rank, world, shuffle, seed, epoch

    def __len__(self):
        return -(-self.n // self.world)

    def __iter__(self):
        if self.shuffle:
            gen = torch.Generator()
            gen.manual_seed((self.seed + 104729 * self.epoch) % (1 << 63))
            order = torch.randperm(self.n, generator=gen).tolist()
        else:
            order = list(range(self.n))
        self.epoch += 1
        per_rank = len(self)
        order = (order * (-(-per_rank * self.world // self.n)))[:per_rank * self.world]
        return iter(order[self.rank::self.world])


class Trainer():
    def __init__(self, model, optimizer, loss=None, dataset=None, batch_size=10,
                 dataloader_kwargs={'num_workers': 2, 'pin_memory': True},
                 valid_split=0.2, num_samples=None, metrics=None, scheduler=None,
                 train_transform=None, valid_transform=None,
                 criterion=None, tr_transform=None, vd_transform=None, sync_every=1, progress=True,
                 capture_step=None):
        self.model = model
        self.optimizer = optimizer
        self.loss = loss if loss is not None else criterion
        if self.loss is None:
            raise TypeError("Trainer needs a loss (loss=... or the legacy criterion=...)")
        self.dataset = dataset
        self.metrics = metrics
        self.scheduler = scheduler
        self.train_transform = train_transform if train_transform is not None else tr_transform
        self.valid_transform = valid_transform if valid_transform is not None else vd_transform
        self.batch_size = batch_size
        self.dataloader_kwargs = {'batch_size': batch_size, **dataloader_kwargs}
        self.num_samples = num_samples
        self.valid_split = valid_split
        self.train_indices, self.valid_indices = [], []
        if dataset is not None:
            self._split_indices()
        self.device = next(model.parameters()).device
        self.best_result = {'loss': float('inf')}
        self.current_epoch = 0
        self.patience_counter = 0
        self.amp_state_dict = None
        self.use_amp = False
        self.save_dir = None
        self.num_epochs = 0
        self.sync_every = max(1, int(sync_every))
        self.progress = progress
        self.progress_bar = _NullBar()
        self._grad_sync = None
        self._scaler = None
        # capture_step: training batches of the usual shape are replayed from a hipGraph of the whole step
        # (graph.GraphedTrainStep - the same kernels on the same data, bit for bit; the host only copies the batch in and
        # one hipGraphLaunch replaces ~500 launches issued from Python).  Needs optim.Adam / AdamW / SGD (their update
        # kernels read the step's scalars from device memory), one process; fp16 storage with its loss scaler only with
        # optim.Adam without max_grad_norm.  None (default): on whenever those hold -
        # with a caller-owned torch.optim.Adam, a loss that is not one of this package's fused losses (a user module may
        # have host-side effects a replay would skip), fp16 loss scaling or several ranks the loop is the eager one, and
        # it stays the fallback if a capture fails.  True: insist (raises when not possible).  False: never.
        self.capture_step = capture_step
        self._graphed = None
        self._capture_failed = False

    # ------------------------------------------------------------------ small helpers
    def _split_indices(self):
        # same draw as the reference: global numpy RNG, floor(valid_split * len) validation cases
        size = len(self.dataset)
        indices = list(range(size))
        split = int(np.floor(self.valid_split * size))
        np.random.shuffle(indices)
        self.train_indices = indices[split:]
        self.valid_indices = indices[:split]

    def get_lr(self, idx=0):
        return self.optimizer.param_groups[idx]['lr']

    def set_lr(self, lr, idx=0):
        self.optimizer.param_groups[idx]['lr'] = lr

    def summary(self, input_shape):
        try:
            from torchsummary import summary as _summary
            return _summary(self.model, input_shape)
        except ImportError:
            total = sum(p.numel() for p in self.model.parameters())
            trainable = sum(p.numel() for p in self.model.parameters() if p.requires_grad)
            text = "%s: %d parameters (%d trainable), input %s" % (type(self.model).__name__, total, trainable,
                                                                   tuple(input_shape))
            print(text)
            return text

    # ------------------------------------------------------------------ the step
    def _flush(self, pending, results):
        """Read back deferred device scalars (one sync for the whole group)."""
        if not pending:
            return None
        keys = list(pending[0].keys())
        stacked = torch.stack([torch.stack([p[k].detach().float().reshape(()) for k in keys]) for p in pending])
        values = stacked.cpu().numpy()
        # the loss kernels' out-of-range label counts travelled in front of these scalars: F.one_hot's error
        # (reference loss.py:27) instead of a silently skipped NaN step, without a sync of its own
        _loss_mod.raise_on_bad_labels()
        last = None
        for row in values:
            result = {k: float(v) for k, v in zip(keys, row)}
            if not math.isnan(result['loss']):
                results.append(result)
            last = result
        pending.clear()
        return last

    def _graphed_step(self):
        if self.capture_step is False or self._capture_failed or self._grad_sync is not None:
            return None
        if self._graphed is None:
            import graph as graph_mod
            import optim as optim_mod
            if not isinstance(self.optimizer, optim_mod._Fused) or self.device.type != 'cuda':
                if self.capture_step:
                    raise TypeError("Trainer(capture_step=True) needs optim.Adam / AdamW / SGD and a model on a HIP device")
                self._capture_failed = True       # auto mode: a caller-owned optimizer keeps the eager loop
                return None
            if self._scaler is not None and not self.optimizer.captures_with_scaler():
                # fp16: only plain optim.Adam has an update kernel that follows the device-side loss scaler
                if self.capture_step:
                    raise TypeError("Trainer(capture_step=True) with fp16 loss scaling needs optim.Adam without "
                                    "max_grad_norm")
                self._capture_failed = True
                return None
            if self.capture_step is None and not isinstance(self.loss, _loss_mod._FusedLoss):
                # auto mode captures only what it knows to be free of host-side effects: a user-defined loss module (one
                # that logs, counts, branches on values) must keep running every step
                self._capture_failed = True
                return None
            self._graphed = graph_mod.GraphedTrainStep(self.model, self.loss, self.optimizer, scaler=self._scaler)
        return self._graphed

    def _release_graph(self):
        """Drop the captured step: its graph holds raw pointers of the optimizer state / gradients it was captured with
        and a private pool with a whole step's activations.  Called whenever those may change (load_checkpoint, a new
        fit() - possibly with another storage type or loss scaler) and when fit() returns."""
        if self._graphed is not None:
            stats = getattr(self, "graph_stats", None) or {"replays": 0, "eager_steps": 0}
            stats["replays"] += self._graphed.replays
            stats["eager_steps"] += self._graphed.eager_steps
            self.graph_stats = stats          # what the captured loop did, for logs and tests
            self._graphed.release()
            self._graphed = None

    def batch_loop(self, data_loader, is_train=True):
        results, pending = [], []
        self.progress_bar.reset(len(data_loader))
        self.progress_bar.set_description("Epoch %d/%d (LR %.2g)" % (self.current_epoch + 1, self.num_epochs,
                                                                     self.get_lr()))
        for batch_idx, batch in enumerate(data_loader):
            x = batch['image'].to(self.device, non_blocking=True)
            y = batch['label'].to(self.device, non_blocking=True)
            graphed = self._graphed_step() if is_train else None
            if graphed is not None:
                self.model.train()
                try:
                    loss = graphed(x, y)
                except Exception:
                    if self.capture_step or graphed.graph is not None:
                        raise
                    # auto mode and the capture itself failed (an op that cannot be captured): eager from here on
                    # (release(): optimizer and loss scaler must not stay in captured mode - the eager step below uses them)
                    self._capture_failed = True
                    self._release_graph()
                    graphed = None
            if graphed is not None:
                y_pred = graphed.logits
                scalars = {'loss': loss.clone()}         # a static buffer: the next replay overwrites it
                if self.metrics is not None:
                    with torch.no_grad():
                        for key, metric_fn in self.metrics.items():
                            scalars[key] = metric_fn(y_pred, y)
                pending.append({k: (v if torch.is_tensor(v) else torch.tensor(float(v))) for k, v in scalars.items()})
                if len(pending) >= self.sync_every:
                    last = self._flush(pending, results)
                    self.progress_bar.set_postfix(last)
                self.progress_bar.update()
                continue
            if is_train:
                self.model.train()
                y_pred = self.model(x)
            else:
                self.model.eval()
                with torch.no_grad():
                    y_pred = self.model(x)
            loss = self.loss(y_pred, y)
            if is_train:
                self.optimizer.zero_grad()
                if self._grad_sync is not None:
                    self._grad_sync.begin_step()
                if self._scaler is not None:
                    self._scaler.scale(loss).backward()      # reference: amp.scale_loss(loss, optimizer)
                else:
                    loss.backward()
                if self._grad_sync is not None:
                    self._grad_sync.finish_step()
                if self._scaler is not None:
                    self._scaler.step(self.optimizer)        # skipped on overflow, like apex's patched step
                else:
                    self.optimizer.step()
            scalars = {'loss': loss}
            if self.metrics is not None:
                y_main = _loss_mod.main_output(y_pred)      # a deep-supervision net trains on a list: metrics see entry 0
                with torch.no_grad():
                    for key, metric_fn in self.metrics.items():
                        scalars[key] = metric_fn(y_main, y)
            pending.append({k: (v if torch.is_tensor(v) else torch.tensor(float(v))) for k, v in scalars.items()})
            if len(pending) >= self.sync_every:
                last = self._flush(pending, results)
                self.progress_bar.set_postfix(last)
            self.progress_bar.update()
        self._flush(pending, results)

        mean_result = {}
        self._last_batches = len(results)
        if results:
            for key in results[0].keys():
                mean_result[key] = float(np.mean(np.array([r[key] for r in results])))
        else:
            mean_result = {'loss': float('nan')}
        name = 'train' if is_train else 'valid'
        if self.save_dir is not None and SummaryWriter is not None:
            writer = SummaryWriter(self.save_dir)
            for key, value in mean_result.items():
                writer.add_scalar('%s/%s' % (key, name), value, self.current_epoch)
            writer.close()
        return mean_result

    # ------------------------------------------------------------------ one process per GPU
    def _enter_distributed(self):
        """Make the ranks one job (the reference is single-process): rank 0's weights, optimizer hyper-parameters
        and train/valid split everywhere, gradient averaging on, per-rank sample streams.  Idempotent."""
        import torch.distributed as dist
        from parallel import make_grad_sync, broadcast_parameters
        if self._grad_sync is None:
            broadcast_parameters(self.model)
            # all ranks end up on one transport (RCCL when every rank can load it, torch.distributed otherwise)
            on_gpu = self.device.type == 'cuda' and dist.get_backend() != "gloo"
            self._grad_sync = make_grad_sync(self.model, transport=os.environ.get("RU3D_COMM", "rccl" if on_gpu else "torch"))
            # BatchNorm nets: each rank normalises its own sub-batch, as the reference's nn.DataParallel replicas do
            # (trainer.py:531-535; rank 0's running averages are the ones checkpointed); RU3D_SYNC_BN=1 pools the
            # statistics over the ranks instead (SyncBN, ops.set_bn_sync)
            if os.environ.get("RU3D_SYNC_BN", "0") == "1":
                import _ops as ops
                ops.set_bn_sync()
        box = [self.train_indices, self.valid_indices, self.current_epoch]
        dist.broadcast_object_list(box, src=0)
        self.train_indices, self.valid_indices, self.current_epoch = box

    def _epoch_mean_over_ranks(self, result):
        """Every rank must feed the scheduler and the best-checkpoint rule the same numbers: the mean over ALL batches of
        the epoch (sum and count are reduced, not a mean of per-rank means)."""
        if not _dist_ready() or not result:
            return result
        import torch.distributed as dist
        keys = sorted(result.keys())
        count = float(max(getattr(self, "_last_batches", 1), 0))
        vals = torch.tensor([[result[k] for k in keys]], dtype=torch.float64)
        vals = torch.nan_to_num(vals, nan=0.0)
        flags = torch.tensor([[0.0 if math.isnan(result[k]) else count for k in keys]], dtype=torch.float64)
        both = torch.cat([vals * flags, flags]).to(self.device if dist.get_backend() == "nccl" else "cpu")
        dist.all_reduce(both)
        both = both.cpu()
        return {k: (float(both[0, i] / both[1, i]) if both[1, i] > 0 else float('nan')) for i, k in enumerate(keys)}

    # ------------------------------------------------------------------ loaders
    def _loader(self, indices, transform, num_samples, shuffle):
        """One process per GPU: the ranks SHARE an epoch (the reference is one process, so an epoch is num_samples draws
        or one pass over the split, whatever the number of GPUs): rank r draws ceil(num_samples / world) samples from its
        own stream, or takes every world-th case of one common permutation (wrapped to equal length - every rank must
        take the same number of steps, the gradient exchange is collective)."""
        subset = Subset(self.dataset, indices, transform)
        kwargs = dict(self.dataloader_kwargs)
        if not _dist_ready():
            if num_samples is not None:
                sampler = torch.utils.data.RandomSampler(subset, True, num_samples)
                return torch.utils.data.DataLoader(subset, sampler=sampler, **kwargs)
            return torch.utils.data.DataLoader(subset, shuffle=shuffle, **kwargs)
        import torch.distributed as dist
        rank, world = dist.get_rank(), dist.get_world_size()
        base = torch.initial_seed() + 104729 * self.current_epoch
        if num_samples is not None:
            gen = torch.Generator()
            gen.manual_seed((base + 7919 * (rank + 1)) % (1 << 63))      # same split on every rank, different draws
            sampler = torch.utils.data.RandomSampler(subset, True, -(-num_samples // world), generator=gen)
            return torch.utils.data.DataLoader(subset, sampler=sampler, **kwargs)
        n = len(subset)
        if n == 0:
            return torch.utils.data.DataLoader(subset, shuffle=False, **kwargs)
        # a fresh common permutation per epoch (the loader is built once; the sampler counts its own epochs)
        sampler = _RankShardSampler(n, rank, world, shuffle, torch.initial_seed(), self.current_epoch)
        return torch.utils.data.DataLoader(subset, sampler=sampler, **kwargs)

    # ------------------------------------------------------------------ fit
    def fit(self, *args, num_epochs=None, save_dir=None, use_amp=False, opt_level='O1', **legacy):
        """fit(num_epochs=10, save_dir=None, use_amp=False, opt_level='O1')  - current API
        fit(dataset, batch_size=, epochs=, num_samples=, valid_split=, log_dir=, save_dir=, save_last=,
            save_best=, num_workers=, pin_memory=)                          - run_train.py spelling"""
        save_last = legacy.pop('save_last', True)
        save_best = legacy.pop('save_best', True)
        # keep the interpreter's full collection (it walks everything torch imported, ~90 ms) out of the step loop
        gc.collect()
        gc.freeze()
        if args and not isinstance(args[0], (int, np.integer)):
            self.dataset = args[0]
            args = args[1:]
            if 'valid_split' in legacy:
                self.valid_split = legacy.pop('valid_split')
            self._split_indices()
        if args:
            num_epochs = args[0]
            if len(args) > 1:
                save_dir = args[1]
        if 'epochs' in legacy:
            num_epochs = legacy.pop('epochs')
        if num_epochs is None:
            num_epochs = 10
        if 'batch_size' in legacy:
            self.batch_size = legacy.pop('batch_size')
            self.dataloader_kwargs['batch_size'] = self.batch_size
        for key in ('num_workers', 'pin_memory'):
            if key in legacy:
                self.dataloader_kwargs[key] = legacy.pop(key)
        if 'num_samples' in legacy:
            self.num_samples = legacy.pop('num_samples')
        log_dir = legacy.pop('log_dir', None)
        if save_dir is None and log_dir is not None:
            save_dir = log_dir
        if legacy:
            raise TypeError("fit() got unexpected arguments %s" % sorted(legacy))
        if self.dataset is None:
            raise ValueError("Trainer.fit: no dataset (pass dataset= to Trainer or as the first fit() argument)")

        self._release_graph()
        self.num_epochs = num_epochs
        self.use_amp = use_amp
        self.save_dir = save_dir
        if use_amp:
            # reference: amp.initialize(model, optimizer, opt_level=opt_level) - apex O1 patches fp16 convolutions in
            # and scales the loss dynamically.  Here: opt_level 'O1' / 'O2' / 'O3' select fp16 storage with fp32
            # accumulation in the HIP kernels plus optim.LossScaler (apex's schedule); opt_level 'bf16' (an extension,
            # also RU3D_AMP_DTYPE=bf16) selects bf16 storage, which needs no loss scaling.
            import network
            import optim as optim_mod
            level = str(opt_level).lower()
            if level == 'o0':
                amp_dtype = torch.float32
            elif level in ('bf16', 'bfloat16') or os.environ.get('RU3D_AMP_DTYPE', '').lower() in ('bf16', 'bfloat16'):
                amp_dtype = torch.bfloat16
            elif level in ('o1', 'o2', 'o3', 'fp16', 'float16'):
                amp_dtype = torch.float16
            else:
                raise ValueError("Trainer.fit: unknown opt_level %r" % (opt_level,))
            network.set_compute_dtype(self.model, amp_dtype)
            if amp_dtype == torch.float16:
                if self._scaler is None:
                    self._scaler = optim_mod.LossScaler()
                    if isinstance(self.amp_state_dict, dict):
                        self._scaler.load_state_dict(self.amp_state_dict)
            else:
                self._scaler = None
        if _dist_ready():
            self._enter_distributed()
        self.progress_bar = tqdm(total=0) if (tqdm is not None and self.progress) else _NullBar()

        train_loader = self._loader(self.train_indices, self.train_transform, self.num_samples, True)
        valid_loader = None
        if len(self.valid_indices) > 0:
            n_valid = round(self.num_samples * self.valid_split) if self.num_samples is not None else None
            valid_loader = self._loader(self.valid_indices, self.valid_transform, n_valid, False)

        for epoch in range(self.current_epoch, num_epochs):
            self.current_epoch = epoch
            result = self.batch_loop(train_loader, is_train=True)
            if valid_loader is not None:
                result = self.batch_loop(valid_loader, is_train=False)
            result = self._epoch_mean_over_ranks(result)
            if self.scheduler is not None:
                if isinstance(self.scheduler, lr_scheduler.ReduceLROnPlateau):
                    self.scheduler.step(result['loss'])
                else:
                    self.scheduler.step()
            if result['loss'] < self.best_result['loss'] - 1e-3:
                self.best_result = result
                if save_dir is not None and save_best:
                    self.save_checkpoint(save_dir + '-best.pt')
            if save_dir is not None and save_last:
                self.save_checkpoint(save_dir + '-last.pt')
        self.progress_bar.close()
        self._release_graph()
        return self.best_result

    # ------------------------------------------------------------------ checkpoints
    def save_checkpoint(self, file_path):
        checkpoint = {'model_state_dict': self.model.state_dict(),
                      'optimizer_state_dict': self.optimizer.state_dict(),
                      'current_epoch': self.current_epoch,
                      'train_indices': self.train_indices,
                      'valid_indices': self.valid_indices,
                      'best_result': self.best_result}
        if self.scheduler is not None:
            checkpoint['scheduler_state_dict'] = self.scheduler.state_dict()
        if self.use_amp:
            # apex's loss-scaler state in the reference (trainer.py:617-618); bf16 needs none - the key is kept
            checkpoint['amp_state_dict'] = (self._scaler.state_dict() if self._scaler is not None
                                            else (self.amp_state_dict or {'ru3d': 'bf16'}))
        directory = os.path.dirname(file_path)
        if directory:
            os.makedirs(directory, exist_ok=True)
        if not _dist_ready() or torch.distributed.get_rank() == 0:
            torch.save(checkpoint, file_path)

    def load_checkpoint(self, file_path):
        try:
            checkpoint = torch.load(file_path, map_location=self.device, weights_only=False)
        except TypeError:  # older torch without weights_only
            checkpoint = torch.load(file_path, map_location=self.device)
        self._release_graph()       # optimizer.load_state_dict replaces the moment tensors a captured Adam points at
        self.model.load_state_dict(checkpoint['model_state_dict'])
        self.optimizer.load_state_dict(checkpoint['optimizer_state_dict'])
        self.current_epoch = checkpoint['current_epoch'] + 1
        self.train_indices = checkpoint['train_indices']
        self.valid_indices = checkpoint['valid_indices']
        self.best_result = checkpoint['best_result']
        if 'amp_state_dict' in checkpoint:
            self.amp_state_dict = checkpoint['amp_state_dict']
            if self._scaler is not None:
                self._scaler.load_state_dict(self.amp_state_dict)
        if 'scheduler_state_dict' in checkpoint and self.scheduler is not None:
            self.scheduler.load_state_dict(checkpoint['scheduler_state_dict'])

    # run_train.py spelling
    save = save_checkpoint
    load = load_checkpoint


# ---------------------------------------------------------------------------------------------------------------------
# Case-level drivers around predict_case (reference trainer.py:136-400): host glue, the arithmetic is in inference.py.
def batch_predict_case(load_dir, save_dir, model, target_spacing, normalize_stats, num_classes=3,
                       patch_size=(240, 240, 80), step_per_patch=4, data_range=None, *,
                       groups=None, group_labels=None, threshold=0.5,
                       placement='reference', weighting='uniform', mirror_axes=(), sigma_scale=0.125):
    """trainer.py:136-161.  `model` may be a list (an ensemble); the keyword-only options are predict_per_patch's."""
    from data import CaseDataset, save_pred
    cases = CaseDataset(load_dir)
    for i in (data_range if data_range is not None else range(len(cases))):
        case = predict_case(cases[i], model, target_spacing, normalize_stats, num_classes, patch_size,
                            step_per_patch, False, placement=placement, weighting=weighting,
                            mirror_axes=mirror_axes, sigma_scale=sigma_scale, groups=groups, group_labels=group_labels,
                            threshold=threshold)
        save_pred(case, save_dir)


def cascade_predict_case(case, coarse_model, coarse_target_spacing, coarse_normalize_stats, coarse_patch_size,
                         detail_model, detail_target_spacing, detail_normalize_stats, detail_patch_size,
                         num_classes=3, step_per_patch=4, region_threshold=10000, crop_padding=20, verbose=True,
                         *, return_device=False, post_transform=None, on_device=None):
    """trainer.py:164-245: a single-class coarse pass finds the regions of interest, the detail model predicts class
    probabilities inside each (padded) region, the regions' maps are averaged where they overlap and arg-maxed.

    on_device: keep the case in HBM between the stages - the image is uploaded once, the coarse mask is labelled and its
    regions are cropped on the device, every region's probability map is added into device `total` / `hits` volumes
    (float64, like the host arithmetic) and only the final uint8 mask is downloaded.  None: yes when both models live on
    a HIP device, unless RU3D_CASCADE_DEVICE=0.  False: the reference's host glue (scipy labelling, numpy merge).  Both
    routes return the same dict.  The arguments up to `verbose` are the reference's, in its order; what this code base
    added behind them is passed by keyword.

    post_transform: any callable volume -> volume (e.g. `functools.partial(transform.post_transform, threshold=t)`),
    applied to the merged mask - on the device route while it is still in HBM (a uint8 HIP tensor in), on the host route
    to the numpy mask.  return_device: leave case['pred'] on the device as a uint8 HIP tensor (device route only; the
    host route has no device copy to return and raises).

    Blending options (placement / weighting / mirror_axes / sigma_scale of predict_per_patch) and ensembles: this
    function's parameter list is the reference's plus the three keywords above and stays that way, so the options ride
    on the model arguments - `inference.Blended(model_or_list, placement='cover', weighting='gaussian', ...)` for
    either stage (usually both).  A plain list or tuple of models is an ensemble with the default options."""
    from data import regions_crop_case
    from inference import Blended
    if isinstance(coarse_model, (list, tuple)):
        coarse_model = Blended(coarse_model)
    if isinstance(detail_model, (list, tuple)):
        detail_model = Blended(detail_model)
    if on_device is None:
        on_device = _models_on_hip(coarse_model, detail_model) and os.environ.get("RU3D_CASCADE_DEVICE", "1") != "0"
    if return_device and not on_device:
        raise ValueError("cascade_predict_case: return_device=True needs the device route (on_device); the host route "
                         "keeps nothing in HBM")
    if on_device:
        return _cascade_predict_case_device(case, coarse_model, coarse_target_spacing, coarse_normalize_stats,
                                            coarse_patch_size, detail_model, detail_target_spacing,
                                            detail_normalize_stats, detail_patch_size, step_per_patch, region_threshold,
                                            crop_padding, verbose, return_device, post_transform)
    if verbose:
        print('Predicting the rough shape for further prediction...')
    case = predict_case(case, coarse_model, coarse_target_spacing, coarse_normalize_stats, 1, coarse_patch_size,
                        step_per_patch, verbose=verbose)
    regions = regions_crop_case(case, region_threshold, crop_padding, 'pred')
    num_classes = detail_model.out_channels
    orig_shape = case['image'].shape[:-1]
    total = np.zeros(list(orig_shape) + [num_classes])
    hits = np.zeros_like(total)
    if verbose:
        print('Cropping regions (%d)...' % len(regions))
    for idx, region in enumerate(regions):
        bbox, shape = region['bbox'], region['image'].shape[:-1]
        if verbose:
            print('Region {} {} predicting...'.format(idx, shape))
        region = predict_case(region, detail_model, detail_target_spacing, detail_normalize_stats, num_classes,
                              detail_patch_size, step_per_patch, verbose=verbose, one_hot=True)
        inside = tuple(slice(max(-bbox[d][0], 0), shape[d] - max(bbox[d][1] - orig_shape[d], 0)) for d in range(3))
        target = tuple(slice(max(bbox[d][0], 0), min(bbox[d][1], orig_shape[d])) for d in range(3))
        total[target] += region['pred'][inside]
        hits[target] += 1
    if verbose:
        print('Merging all regions...')
    seen = hits > 0
    total[seen] = total[seen] / hits[seen]
    if num_classes == 1:
        merged = np.around(np.squeeze(total, axis=-1))
    else:
        e = np.exp(total - total.max(axis=-1, keepdims=True))      # scipy.special.softmax, then argmax
        merged = np.argmax(e / e.sum(axis=-1, keepdims=True), axis=-1)
    case['pred'] = merged.astype(np.uint8)
    if post_transform is not None:
        case['pred'] = post_transform(case['pred'])
    if verbose:
        print('All done!')
    return case


def _models_on_hip(*models):
    for m in models:
        p = next(m.parameters(), None)
        if p is None or not p.is_cuda:
            return False
    return True


def _cascade_predict_case_device(case, coarse_model, coarse_target_spacing, coarse_normalize_stats, coarse_patch_size,
                                 detail_model, detail_target_spacing, detail_normalize_stats, detail_patch_size,
                                 step_per_patch, region_threshold, crop_padding, verbose, return_device=False,
                                 post_transform=None):
    """cascade_predict_case with every intermediate in HBM (components.py, csrc/components.hip)."""
    import components
    from data import regions_crop_case
    device = next(coarse_model.parameters()).device
    if next(detail_model.parameters()).device != device:
        raise ValueError("cascade_predict_case(on_device=True): the two models live on %s and %s"
                         % (device, next(detail_model.parameters()).device))
    image = case['image'] if torch.is_tensor(case['image']) else np.asarray(case['image'])
    if image.ndim == 3:
        image = image[..., None]
    if torch.is_tensor(image):
        dev_image = image.to(device=device, dtype=torch.float32)
    else:
        dev_image = torch.from_numpy(np.ascontiguousarray(image, dtype=np.float32)).to(device)
    if verbose:
        print('Predicting the rough shape for further prediction...')
    work = dict(case)
    work['image'] = dev_image
    work = predict_case(work, coarse_model, coarse_target_spacing, coarse_normalize_stats, 1, coarse_patch_size,
                        step_per_patch, verbose=verbose, return_device=True)
    regions = regions_crop_case(work, region_threshold, crop_padding, 'pred')
    num_classes = detail_model.out_channels
    orig_shape = tuple(int(v) for v in dev_image.shape[:-1])
    acc = components.CascadeAccumulator(orig_shape, num_classes, device)
    if verbose:
        print('Cropping regions (%d)...' % len(regions))
    for idx, region in enumerate(regions):
        bbox = region['bbox']
        if verbose:
            print('Region {} {} predicting...'.format(idx, tuple(region['image'].shape[:-1])))
        region = predict_case(region, detail_model, detail_target_spacing, detail_normalize_stats, num_classes,
                              detail_patch_size, step_per_patch, verbose=verbose, one_hot=True, return_device=True)
        acc.add(region['pred'], bbox[:, 0])
    if verbose:
        print('Merging all regions...')
    pred = acc.merge()
    if post_transform is not None:
        pred = post_transform(pred)
    case['pred'] = pred if return_device or not torch.is_tensor(pred) else pred.cpu().numpy()
    case['affine'] = work['affine']
    if verbose:
        print('All done!')
    return case


def cascade_predict(image_file, coarse_model, coarse_target_spacing, coarse_normalize_stats, coarse_patch_size,
                    detail_model, detail_target_spacing, detail_normalize_stats, detail_patch_size, air=-200, num_classes=3,
                    step_per_patch=4, region_threshold=10000, crop_padding=20, label_file=None, verbose=True,
                    on_device=None, post_transform=None):
    """trainer.py:248-302: load a NIfTI image, reorient + crop it to its non-air box, run the cascade on the crop, and
    put the mask back into a volume of the original file's grid.  As in the reference the final step applies the
    forward orientation once more (`apply_orientation(orig_pred, orient)`), which undoes the first one for the
    orientations that are their own inverse - every pure flip, and the usual axis swaps.

    post_transform (a callable volume -> volume) is applied by cascade_predict_case to the mask of the cropped,
    re-oriented case - before that mask is pasted into the file's grid, so a size threshold or a structure is in the
    crop's voxels and the volume's faces (the border rule of a closing) are the crop's faces."""
    from data import apply_orientation, io_orientation, load_case, orient_crop_case
    orig_case = load_case(image_file, label_file)
    case = orient_crop_case(orig_case, air)
    case = cascade_predict_case(case, coarse_model, coarse_target_spacing, coarse_normalize_stats, coarse_patch_size,
                                detail_model, detail_target_spacing, detail_normalize_stats, detail_patch_size,
                                num_classes, step_per_patch, region_threshold, crop_padding, verbose,
                                on_device=on_device, post_transform=post_transform)
    ornt = io_orientation(orig_case['affine'])
    order = ornt[:, 0].astype(int)
    orig_shape = np.take(np.array(orig_case['image'].shape[:3]), order)
    bbox = case['bbox']
    orig_pred = np.zeros(orig_shape, dtype=np.uint8)
    target = tuple(slice(max(bbox[d][0], 0), min(bbox[d][1], orig_shape[d])) for d in range(3))
    orig_pred[target] = case['pred']
    orig_case['pred'] = apply_orientation(orig_pred, ornt)
    if orig_case['image'].ndim == 3:
        orig_case['image'] = np.expand_dims(orig_case['image'], -1)
    return orig_case


def batch_cascade_predict(image_dir, save_dir, coarse_model, coarse_target_spacing, coarse_normalize_stats,
                          coarse_patch_size, detail_model, detail_target_spacing, detail_normalize_stats,
                          detail_patch_size, air=-200, num_classes=3, step_per_patch=4, region_threshold=10000,
                          crop_padding=20, data_range=None, on_device=None, post_transform=None):
    """trainer.py:305-345: every file of `image_dir` through cascade_predict, masks written with save_pred.
    post_transform: see cascade_predict (applied to the cropped, re-oriented mask of every file)."""
    from pathlib import Path
    from data import save_pred
    image_files = [path for path in sorted(Path(image_dir).iterdir()) if path.is_file()]
    for i in (data_range if data_range is not None else range(len(image_files))):
        case = cascade_predict(image_files[i], coarse_model, coarse_target_spacing, coarse_normalize_stats,
                               coarse_patch_size, detail_model, detail_target_spacing, detail_normalize_stats,
                               detail_patch_size, air, num_classes, step_per_patch, region_threshold, crop_padding,
                               None, False, on_device, post_transform)
        save_pred(case, save_dir)


_EVAL_CLASSES = 32          # the device table tells classes 0 .. 31 apart; row / column 32 collects everything above


def _is_hip(v):
    return torch.is_tensor(v) and v.is_cuda


def _device_bytes(v, device):
    """uint8 HIP tensor of a label volume (numpy or tensor, any integer type; values above 255 stay above 31)."""
    if torch.is_tensor(v):
        return v.to(device) if v.dtype == torch.uint8 else v.to(device).clamp(0, 255).to(torch.uint8)
    v = np.asarray(v)
    if v.dtype != np.uint8:
        v = np.clip(v, 0, 255).astype(np.uint8)
    return torch.from_numpy(np.ascontiguousarray(v)).to(device)


def _ignore_to_row(label, ig):
    """(label volume for _device_bytes, count of its ignore voxels, table row that collects them) for an ignore label
    ig.  A value in 0 .. 31 has its own row; any other is mapped to 255 BEFORE _device_bytes clamps - a negative value
    must not be clamped to background - and lands in row 32.  The count of a HIP volume stays on the device."""
    if torch.is_tensor(label):
        hit = label == ig
        count = hit.sum()
        if not 0 <= ig < _EVAL_CLASSES and ig != 255:
            label = torch.where(hit, torch.full((), 255, dtype=torch.int64, device=label.device), label.long())
    else:
        label = np.asarray(label)
        hit = label == ig
        count = int(hit.sum())
        if not 0 <= ig < _EVAL_CLASSES and ig != 255:
            label = np.where(hit, 255, label.astype(np.int64))
    return label, count, (ig if 0 <= ig < _EVAL_CLASSES else _EVAL_CLASSES)


def _confusion_table(case, ignore_label=None):
    """(int64 numpy table [K, K] with entry [l][p] = voxels of label l predicted as p, highest label present).
    HIP operands: one launch of the confusion kernel (the other operand is uploaded if needed) and one download of the
    33 x 33 table; numpy operands: one np.bincount.  ignore_label: voxels whose LABEL has this value count in no cell
    (numpy: masked before the bincount; HIP: their row is dropped, and their count comes down with the table)."""
    pred, label = case['pred'], case['label']
    if _is_hip(pred) or _is_hip(label):
        import morphology
        device = pred.device if _is_hip(pred) else label.device
        row = None
        if ignore_label is not None:
            label, ignored, row = _ignore_to_row(label, int(ignore_label))
        table = morphology.confusion(_device_bytes(pred, device), _device_bytes(label, device), _EVAL_CLASSES)
        if row is not None and torch.is_tensor(ignored):      # one download: the table, then the count
            both = torch.cat([table.reshape(-1), ignored.to(table.device).reshape(1).to(table.dtype)]).cpu().numpy()
            table, ignored = both[:-1].reshape(tuple(table.shape)).copy(), int(both[-1])
        else:
            table = table.cpu().numpy()
        if row is not None:
            if row < _EVAL_CLASSES or int(table[row].sum()) <= ignored:      # else: a class above 31 beside the ignored
                table[row, :] = 0
        present = np.flatnonzero(table.sum(axis=1))
        top = int(present.max()) if present.size else 0
        if top >= _EVAL_CLASSES:
            raise ValueError("evaluate: case['label'] holds a class above %d; the device table tells classes 0 .. %d apart"
                             % (_EVAL_CLASSES - 1, _EVAL_CLASSES - 1))
        return table, top
    pred = np.asarray(pred.cpu() if torch.is_tensor(pred) else pred).astype(np.int64).ravel()
    label = np.asarray(label.cpu() if torch.is_tensor(label) else label).astype(np.int64).ravel()
    if ignore_label is not None:
        keep = label != int(ignore_label)
        pred, label = pred[keep], label[keep]
        if label.size == 0:
            return np.zeros((1, 1), dtype=np.int64), 0
    top = int(label.max())
    k = max(top, int(pred.max())) + 1
    return np.bincount(label * k + pred, minlength=k * k).reshape(k, k), top


def _class_counts(table, c):
    """true positives, false negatives, false positives, true negatives of class c as Python ints."""
    tp = int(table[c, c])
    fn = int(table[c].sum()) - tp
    fp = int(table[:, c].sum()) - tp
    return tp, fn, fp, int(table.sum()) - tp - fn - fp


def evaluate_case(case, ignore_label=None):
    """trainer.py:348-356: Dice (loss.dice, alpha = beta = 0.5) of every foreground class of label vs pred.  When the
    prediction or the label is a HIP tensor the Dice values come from the integer confusion table of the two volumes
    (one kernel launch, csrc/morphology.hip) in Python floats.  ignore_label: voxels whose label has this value count
    nowhere - not in tp, fn, fp or tn - and the classes run up to the highest label among the others."""
    if _is_hip(case['pred']) or _is_hip(case['label']):
        table, top = _confusion_table(case, ignore_label)
        out = []
        for c in range(1, top + 1):
            tp, fn, fp, _ = _class_counts(table, c)
            out.append((tp + 1e-7) / (tp + 0.5 * fn + 0.5 * fp + 1e-7))
        return out
    out = []
    if ignore_label is not None:
        keep = np.asarray(case['label']) != int(ignore_label)
        case = {'pred': np.asarray(case['pred'])[keep], 'label': np.asarray(case['label'])[keep]}
        if case['label'].size == 0:
            return out
    for c in range(int(case['label'].max())):
        p = np.array(case['pred'] == c + 1).astype(np.float32)
        g = np.array(case['label'] == c + 1).astype(np.float32)
        out.append(dice(torch.tensor(p), torch.tensor(g)).item())
    return out


def evaluate_metrics(case, smooth=1e-7, ignore_label=None):
    """Dice, sensitivity, specificity and accuracy (the formulas of the reference's nb.py:11-25) of every foreground
    class 1 .. label.max(): a list of dicts with the keys dsc / sen / spe / acc.  All four are functions of one table
    of integer counts - np.bincount on numpy volumes, the confusion kernel when either volume is a HIP tensor.
    ignore_label: voxels whose label has this value count in no cell of that table."""
    table, top = _confusion_table(case, ignore_label)
    out = []
    for c in range(1, top + 1):
        tp, fn, fp, tn = _class_counts(table, c)
        out.append({'dsc': (tp + smooth) / (tp + 0.5 * (fn + fp) + smooth),
                    'sen': (tp + smooth) / (tp + fn + smooth),
                    'spe': (tn + smooth) / (tn + fp + smooth),
                    'acc': (tp + tn + smooth) / (tp + tn + fn + fp + smooth)})
    return out


def evaluate_groups_case(case, groups, smooth=1e-7):
    """Dice of every label group between case['label'] and case['pred'], both label maps: a voxel is in group k iff its
    label is a member of groups[k], so a whole organ is scored as one structure beside the structure nested inside it.
    A list of len(groups) floats, (tp + smooth) / (tp + 0.5 fn + 0.5 fp + smooth) from the integer confusion table of
    the two volumes (np.bincount on numpy volumes, the confusion kernel when either is a HIP tensor); a group absent
    from both maps scores smooth / smooth = 1."""
    gs, _ = _loss_mod._checked_groups(groups)
    table, _ = _confusion_table(case)
    out = []
    for g in gs:
        members = [t for t in g if t < table.shape[0]]
        tp = int(table[np.ix_(members, members)].sum())
        fn = int(table[members, :].sum()) - tp
        fp = int(table[:, members].sum()) - tp
        out.append((tp + smooth) / (tp + 0.5 * fn + 0.5 * fp + smooth))
    return out


def evaluate_groups(label_file, pred_file, groups):
    """evaluate for label groups: evaluate_groups_case of two NIfTI label maps."""
    import nifti
    label, _, _ = nifti.load(label_file)
    pred, _, _ = nifti.load(pred_file)
    return evaluate_groups_case({'label': label.astype(np.uint8), 'pred': pred.astype(np.uint8)}, groups)


def batch_evaluate_groups(label_dir, pred_dir, groups, data_range=None):
    """batch_evaluate for label groups: one list of len(groups) Dice values per case, the means printed."""
    from pathlib import Path
    label_files = sorted(Path(label_dir).glob('*.nii.gz'))
    pred_files = sorted(Path(pred_dir).glob('*.nii.gz'))
    results = [evaluate_groups(label_files[i], pred_files[i], groups)
               for i in (data_range if data_range is not None else range(len(label_files)))]
    print('\nThe mean dsc of each group:')
    for i, m in enumerate(np.array(results).mean(axis=0)):
        print("group_%d %s: %f" % (i, tuple(groups[i]), m))
    return results


def evaluate(label_file, pred_file):
    """trainer.py:359-368"""
    import nifti
    label, _, _ = nifti.load(label_file)
    pred, _, _ = nifti.load(pred_file)
    return evaluate_case({'label': label.astype(np.uint8), 'pred': pred.astype(np.uint8)})


def batch_evaluate(label_dir, pred_dir, data_range=None):
    """trainer.py:371-400"""
    from pathlib import Path
    label_files = sorted(Path(label_dir).glob('*.nii.gz'))
    pred_files = sorted(Path(pred_dir).glob('*.nii.gz'))
    results = [evaluate(label_files[i], pred_files[i])
               for i in (data_range if data_range is not None else range(len(label_files)))]
    print('\nThe mean dsc of each label:')
    for i, m in enumerate(np.array(results).mean(axis=0)):
        print("label_%d: %f" % (i + 1, m))
    return results


# ------------------------------------------------------------------ surface-distance metrics
def _spacing3(spacing, ndim):
    """`spacing` (None = 1 per axis) as three floats for a volume of 1 to 3 axes, leading axes of length 1 first."""
    if not 1 <= ndim <= 3:
        raise ValueError("evaluate_surface_case: a volume of %d axes (1 to 3)" % ndim)
    s = (1.0,) * ndim if spacing is None else tuple(float(v) for v in spacing)
    if len(s) != ndim or not all(math.isfinite(v) and v > 0 for v in s):
        raise ValueError("evaluate_surface_case: spacing=%r for a volume of %d axes (one finite value > 0 per axis)"
                         % (spacing, ndim))
    return (1.0,) * (3 - ndim) + s


def _nearest_feature_numpy(features, spacing):
    """scipy's feature transform: int32 [3, X, Y, Z], the index of the nearest set voxel of `features` (not empty)."""
    import scipy.ndimage as ndi
    return ndi.distance_transform_edt(~features, sampling=spacing, return_distances=False, return_indices=True)


def _contract_sq_numpy(src, nearest, spacing):
    """Squared distances from the set voxels of `src` (element order) to the voxels `nearest` names for them, through
    the expression the device transform is held to: fl(A + fl(B + C)) with A = fl(fl(sx (px - fx))^2), in float64 - not
    the square of scipy's rooted output."""
    at = np.nonzero(src)
    a, b, c = ((spacing[k] * (at[k] - nearest[k][at]).astype(np.float64)) ** 2 for k in range(3))
    return a + (b + c)


def _surface_reduce_numpy(d_ab, d_ba, tolerance):
    """The reductions of distance.surface_stats over two non-empty vectors of squared distances."""
    tol_sq = float(tolerance) * float(tolerance)
    lo, hi = _percentile_ranks(d_ab.size + d_ba.size)
    both = np.partition(np.concatenate((d_ab, d_ba)), (lo, hi))
    return dict(n_ab=int(d_ab.size), n_ba=int(d_ba.size),
                max_ab=float(d_ab.max()), within_ab=int((d_ab <= tol_sq).sum()), sum_ab=float(np.sqrt(d_ab).sum()),
                max_ba=float(d_ba.max()), within_ba=int((d_ba <= tol_sq).sum()), sum_ba=float(np.sqrt(d_ba).sum()),
                lo=float(both[lo]), hi=float(both[hi]))


def _surface_numpy(mask):
    import scipy.ndimage as ndi
    return mask & ~ndi.binary_erosion(mask)


def _surface_stats_numpy(a, b, spacing, tolerance):
    """distance.surface_stats on the host: the same dict from two boolean volumes [X, Y, Z]."""
    sa, sb = _surface_numpy(a), _surface_numpy(b)
    if not sa.any() or not sb.any():
        return {'n_ab': int(sa.sum()), 'n_ba': int(sb.sum())}
    return _surface_reduce_numpy(_contract_sq_numpy(sa, _nearest_feature_numpy(sb, spacing), spacing),
                                 _contract_sq_numpy(sb, _nearest_feature_numpy(sa, spacing), spacing), tolerance)


def _percentile_ranks(n, q=95.0):
    """The two zero-based order statistics np.percentile(., q) interpolates between for n values (its default, linear)."""
    lo = int(math.floor(q / 100.0 * (n - 1)))
    return lo, min(lo + 1, n - 1)


def _surface_metrics(stats, q=95.0):
    """hd / hd95 / assd / nsd from the dict of distance.surface_stats (or its host twin).  The square root is taken
    here, on a handful of numbers; the percentile is np.percentile's linear interpolation written out."""
    n_ab, n_ba = stats['n_ab'], stats['n_ba']
    if n_ab == 0 and n_ba == 0:
        return {'hd': 0.0, 'hd95': 0.0, 'assd': 0.0, 'nsd': 1.0}
    if n_ab == 0 or n_ba == 0:
        return {'hd': math.inf, 'hd95': math.inf, 'assd': math.inf, 'nsd': 0.0}
    n = n_ab + n_ba
    lo, hi = math.sqrt(stats['lo']), math.sqrt(stats['hi'])
    gamma = q / 100.0 * (n - 1) - _percentile_ranks(n, q)[0]
    hd95 = hi - (hi - lo) * (1 - gamma) if gamma >= 0.5 else lo + (hi - lo) * gamma
    return {'hd': math.sqrt(max(stats['max_ab'], stats['max_ba'])),
            'hd95': hd95,
            'assd': (stats['sum_ab'] / n_ab + stats['sum_ba'] / n_ba) / 2,
            'nsd': (stats['within_ab'] + stats['within_ba']) / n}


def _surface_stats_case(case, spacing, tolerance):
    """One dict of surface statistics (distance.surface_stats) per foreground class 1 .. label.max()."""
    pred, label = case['pred'], case['label']
    if tuple(pred.shape) != tuple(label.shape):
        raise ValueError("evaluate_surface_case: pred has shape %s, label %s" % (tuple(pred.shape), tuple(label.shape)))
    spacing = _spacing3(spacing, len(label.shape))
    if float(tolerance) < 0 or math.isnan(float(tolerance)):
        raise ValueError("evaluate_surface_case: tolerance=%r (>= 0)" % (tolerance,))
    if _is_hip(pred) or _is_hip(label):
        import distance
        import morphology
        device = pred.device if _is_hip(pred) else label.device
        pred, label = _device_bytes(pred, device), _device_bytes(label, device)
        top = int(label.max().item()) if label.numel() else 0
        sampling = spacing[3 - label.dim():]
        return [distance.surface_stats(morphology.pack(pred, 'eq', c), morphology.pack(label, 'eq', c), sampling, tolerance)
                for c in range(1, top + 1)]
    pred = np.asarray(pred.cpu() if torch.is_tensor(pred) else pred)
    label = np.asarray(label.cpu() if torch.is_tensor(label) else label)
    shape3 = (1,) * (3 - label.ndim) + label.shape
    pred, label = pred.reshape(shape3), label.reshape(shape3)
    top = int(label.max()) if label.size else 0
    return [_surface_stats_numpy(pred == c, label == c, spacing, tolerance) for c in range(1, top + 1)]


def evaluate_surface_case(case, spacing=None, tolerance=1.0):
    """Boundary metrics of every foreground class 1 .. label.max(): a list of dicts with the keys
      hd    Hausdorff distance: the largest distance from a surface voxel of one mask to the other mask's surface,
      hd95  np.percentile(., 95) of all those distances (both directions concatenated),
      assd  average symmetric surface distance: the mean of the two directions' mean distances,
      nsd   surface Dice at `tolerance`: the share of surface voxels (of both masks) within the tolerance of the other
            surface, decided on the squared distances in float64.
    A mask's surface is `mask & ~binary_erosion(mask)` (6-neighbour cross, the volume's faces count as outside) and
    distances are Euclidean between voxel centres in `spacing` units (None: 1 per axis).  Both masks empty gives
    0, 0, 0, 1; exactly one empty gives inf, inf, inf, 0.  numpy operands run on the host (scipy); when `pred` or
    `label` is a HIP tensor the other operand is uploaded and surfaces, distance transforms (csrc/distance.hip),
    gathers and reductions stay on the device: per class one download of ten numbers."""
    return [_surface_metrics(s) for s in _surface_stats_case(case, spacing, tolerance)]


def evaluate_surface(label_file, pred_file, tolerance=1.0, device=None):
    """evaluate_surface_case of two NIfTI files, with the spacing of the label's affine.  device: a HIP device uploads
    both volumes (as bytes) and evaluates there."""
    import nifti
    from data import get_spacing
    label, affine, _ = nifti.load(label_file)
    pred, _, _ = nifti.load(pred_file)
    case = {'label': label.astype(np.uint8), 'pred': pred.astype(np.uint8)}
    if device is not None:
        case = {k: torch.from_numpy(np.ascontiguousarray(v)).to(device) for k, v in case.items()}
    return evaluate_surface_case(case, spacing=get_spacing(affine), tolerance=tolerance)


def batch_evaluate_surface(label_dir, pred_dir, data_range=None, tolerance=1.0, device=None):
    """evaluate_surface over the sorted *.nii.gz files of two directories; prints the mean of each metric per class
    (over the cases that have the class) and returns the per-case lists."""
    from pathlib import Path
    label_files = sorted(Path(label_dir).glob('*.nii.gz'))
    pred_files = sorted(Path(pred_dir).glob('*.nii.gz'))
    results = [evaluate_surface(label_files[i], pred_files[i], tolerance, device)
               for i in (data_range if data_range is not None else range(len(label_files)))]
    for key in ('hd', 'hd95', 'assd', 'nsd'):
        print('\nThe mean %s of each label:' % key)
        for c in range(max((len(r) for r in results), default=0)):
            print("label_%d: %f" % (c + 1, np.mean([r[c][key] for r in results if len(r) > c])))
    return results


# ------------------------------------------------------------------ surface meshes of the predicted structures
def _mesh_labels(labels, top):
    """[(name, (values ...)), ...]: None = every value 1 .. top; an entry may be a tuple, meaning the union of its
    values (kidney and tumour = (1, 2))."""
    if labels is None:
        labels = range(1, top + 1)
    out = []
    for entry in labels:
        values = tuple(int(v) for v in entry) if isinstance(entry, (tuple, list)) else (int(entry),)
        if not values or any(v < 1 or v > 255 for v in values):
            raise ValueError("extract_mesh_case: label %r (values 1 .. 255, or a tuple of them)" % (entry,))
        out.append((tuple(entry) if isinstance(entry, (tuple, list)) else int(entry), values))
    return out


def extract_mesh_case(case, labels=None, key='pred', smooth_iterations=10, lam=0.5, mu=-0.53, return_device=False):
    """One closed triangle mesh per structure of the label volume `case[key]`: a list of dicts
      label     the value (or the tuple of values whose union was meshed),
      vertices  float64 [V, 3] in the world coordinates of `case['affine']` (millimetres; voxel coordinates without one),
      faces     int32 [F, 3], counter-clockwise seen from outside (also under an affine that mirrors),
      area, volume   of the mesh in those units (mm^2, mm^3).
    The surface is the voxels' own faces (transform.extract_mesh), Taubin-smoothed in index space; the affine is applied
    afterwards and the measures are taken on the world positions.  labels=None means every value 1 .. max.  A numpy
    volume takes the numpy route.  A HIP volume - for instance `cascade_predict_case(..., return_device=True)['pred']` -
    is packed, meshed, smoothed, mapped and measured on the device (csrc/mesh.hip); what is downloaded is the finished
    vertices and faces, or with return_device=True only the two measures."""
    import transform
    volume = case[key]
    affine = np.asarray(case['affine'], dtype=np.float64) if case.get('affine') is not None else np.eye(4)
    results = []
    if _is_hip(volume):
        import mesh
        import morphology
        if volume.dim() < 1 or volume.dim() > 3:
            raise ValueError("extract_mesh_case: case[%r] has shape %s (1 to 3 axes)" % (key, tuple(volume.shape)))
        volume = _device_bytes(volume, volume.device)
        top = int(volume.max().item()) if labels is None else 0
        for name, values in _mesh_labels(labels, top):
            packed = morphology.pack(volume, 'eq', values[0])
            for v in values[1:]:
                packed.bits |= morphology.pack(volume, 'eq', v).bits
            m = mesh.smooth(mesh.extract(packed), smooth_iterations, lam, mu)
            vertices, faces = mesh.to_world(m.vertices, affine, m.faces)
            area, vol = mesh.measure(vertices, faces).tolist()
            if not return_device:
                vertices, faces = vertices.cpu().numpy(), faces.cpu().numpy()
            results.append({'label': name, 'vertices': vertices, 'faces': faces, 'area': area, 'volume': vol})
        return results
    volume = np.asarray(volume.cpu() if torch.is_tensor(volume) else volume)
    if volume.ndim < 1 or volume.ndim > 3:
        raise ValueError("extract_mesh_case: case[%r] has shape %s (1 to 3 axes)" % (key, volume.shape))
    top = int(volume.max()) if labels is None and volume.size else 0
    for name, values in _mesh_labels(labels, top):
        m = transform.extract_mesh(np.isin(volume, values), smooth_iterations, lam, mu)
        vertices, faces = transform._to_world_numpy(m.vertices, m.faces, affine)
        area, vol = transform._measure_mesh_numpy(vertices, faces)
        results.append({'label': name, 'vertices': vertices, 'faces': faces, 'area': area, 'volume': vol})
    return results


def _label_name(label):
    return '_'.join(str(v) for v in label) if isinstance(label, tuple) else str(label)


def extract_mesh(pred_file, save_dir=None, fmt='stl', device=None, labels=None, smooth_iterations=10, lam=0.5, mu=-0.53):
    """extract_mesh_case of a NIfTI label volume (a `*.pred.nii.gz` of save_pred, or a ground-truth segmentation) with
    the file's affine.  save_dir: every non-empty structure is written as `<case_id>.label_<n>.<fmt>` (fmt 'stl' or
    'ply'; a union (1, 2) is named label_1_2) and its dict gains 'file'.  device: a HIP device uploads the volume (as
    bytes) and meshes there.  Prints volume (ml) and area (mm^2) per structure; returns the list of dicts."""
    import nifti
    import meshfile
    from pathlib import Path
    if fmt not in meshfile.WRITERS:
        raise ValueError("extract_mesh: fmt=%r ('stl' or 'ply')" % (fmt,))
    pred_file = Path(pred_file)
    case_id = pred_file.name
    for suffix in ('.gz', '.nii', '.pred'):
        if case_id.endswith(suffix):
            case_id = case_id[:-len(suffix)]
    pred, affine, _ = nifti.load(pred_file)
    pred = np.ascontiguousarray(np.clip(pred, 0, 255).astype(np.uint8))
    case = {'case_id': case_id, 'affine': affine, 'pred': pred if device is None else torch.from_numpy(pred).to(device)}
    results = extract_mesh_case(case, labels, 'pred', smooth_iterations, lam, mu)
    if save_dir is not None:
        save_dir = Path(save_dir)
        save_dir.mkdir(parents=True, exist_ok=True)
    for r in results:
        print("%s label_%s: volume %.3f ml, area %.1f mm^2, %d vertices, %d triangles"
              % (case_id, _label_name(r['label']), r['volume'] / 1000.0, r['area'], len(r['vertices']), len(r['faces'])))
        if save_dir is not None and len(r['faces']):
            r['file'] = save_dir / ('%s.label_%s.%s' % (case_id, _label_name(r['label']), fmt))
            meshfile.WRITERS[fmt](r['file'], r['vertices'], r['faces'])
    return results


def batch_extract_mesh(pred_dir, save_dir, data_range=None, fmt='stl', device=None, labels=None, smooth_iterations=10,
                       lam=0.5, mu=-0.53):
    """extract_mesh over the sorted *.nii.gz files of `pred_dir`; returns the per-file lists."""
    from pathlib import Path
    pred_files = sorted(Path(pred_dir).glob('*.nii.gz'))
    return [extract_mesh(pred_files[i], save_dir, fmt, device, labels, smooth_iterations, lam, mu)
            for i in (data_range if data_range is not None else range(len(pred_files)))]


# ------------------------------------------------------------------ morphometry: the numbers of a report
def _entry_mask(volume, values):
    """uint8 0 / 1 volume of the voxels of `volume` (numpy or HIP, uint8) that carry one of `values`."""
    if torch.is_tensor(volume):
        mask = volume == values[0]
        for v in values[1:]:
            mask |= volume == v
        return mask.view(torch.uint8)
    return np.isin(volume, values).view(np.uint8)


def _entry_components(mask, min_voxels):
    """(int32 labels, K) of the 6-connected components of `mask` with at least `min_voxels` voxels, numbered in the
    order of their first voxel among the survivors (scipy's numbering when nothing is dropped)."""
    import transform
    labels, count = transform.label_components(mask)
    if count == 0 or min_voxels <= 1:
        return labels, count
    if torch.is_tensor(labels):
        import components
        sizes, _ = components.stats(labels, count)
        return components.filter_small(labels, count, sizes, min_voxels, relabel=True)
    keep = np.bincount(labels.ravel(), minlength=count + 1)[1:] >= min_voxels
    remap = np.r_[0, np.where(keep, np.cumsum(keep), 0)].astype(labels.dtype)
    return remap[labels], int(keep.sum())


def measure_case(case, key='pred', labels=None, components=False, min_voxels=0, gaps=(), return_device=False):
    """The morphometry of the label volume `case[key]` (csrc/morphometry.hip, morphometry.describe): a dict with
      case_id     the case's, when it has one,
      structures  one dict per measured structure: `label` (the value, or the tuple of values of a union) and the fields
                  of morphometry.describe - voxels, volume_mm3, centroid, principal axes and their extents, the longest
                  diameter with its end points, surface, contact area per class and exposed fraction - in the world
                  coordinates of `case['affine']` (voxel units without one),
      gaps        one dict per pair of `gaps`: a, b (two label entries) and gap_mm, their smallest distance in mm.
    labels: entries as in extract_mesh_case, None = every non-zero value the volume holds.  components=True splits every entry into its
    6-connected components, drops those below min_voxels and measures each one (`component` = its number in scipy's
    order).  Contact is counted against the class volume itself.  A numpy volume takes the numpy route; a HIP volume -
    for instance `cascade_predict_case(..., return_device=True)['pred']` - never leaves the device: the kernels fill
    small tables and only those are downloaded.  return_device=True downloads nothing: every structure is `label`,
    `count` and the raw tables `moments`, `faces`, `feret_d2`, `feret_pair` where the volume lives."""
    import morphometry
    volume = case[key]
    affine = np.asarray(case['affine'], dtype=np.float64) if case.get('affine') is not None else None
    hip = _is_hip(volume)
    if hip:
        volume = _device_bytes(volume, volume.device)
    else:
        volume = np.asarray(volume.cpu() if torch.is_tensor(volume) else volume)
        if volume.dtype != np.uint8:
            volume = np.clip(volume, 0, 255).astype(np.uint8)
    ndim = volume.dim() if hip else volume.ndim
    if ndim < 1 or ndim > 3:
        raise ValueError("measure_case: case[%r] has shape %s (1 to 3 axes)" % (key, tuple(volume.shape)))
    top = int(volume.max()) if volume.shape and min(volume.shape) > 0 else 0
    if labels is None:                          # every value the volume holds, not every value up to a stray 255
        labels = [v for v in (torch.unique(volume) if hip else np.unique(volume)).tolist() if v >= 1]
    masks = {}

    def mask_of(values):
        if values not in masks:
            masks[values] = _entry_mask(volume, values)
        return masks[values]

    structures = []
    for name, values in _mesh_labels(labels, top):
        ids, count = mask_of(values), 1
        if components:
            ids, count = _entry_components(ids, min_voxels)
        if return_device:
            d2, pair = morphometry.feret(ids, count, morphometry.gram(affine))
            structures.append({'label': name, 'count': count, 'moments': morphometry.moments(ids, count),
                               'faces': morphometry.faces(ids, count, volume, top + 1), 'feret_d2': d2, 'feret_pair': pair})
            continue
        for d in morphometry.describe(ids, count, affine=affine, other=volume, num_other=top + 1):
            d['label'] = name
            if components:
                d['component'] = d['id']
            del d['id']
            structures.append(d)
    A = affine[:3, :3] if affine is not None else np.eye(3)
    sampling = tuple(float(s) for s in np.linalg.norm(A, axis=0)[3 - ndim:])
    found = []
    for a, b in gaps:
        (name_a, values_a), (name_b, values_b) = _mesh_labels((a, b), top)
        found.append({'a': name_a, 'b': name_b, 'gap_mm': morphometry.gap_mm(mask_of(values_a), mask_of(values_b), sampling)})
    result = {'structures': structures, 'gaps': found}
    if 'case_id' in case:
        result['case_id'] = case['case_id']
    return result


def measure(pred_file, save_dir=None, device=None, **options):
    """measure_case of a NIfTI label volume (a `*.pred.nii.gz` of save_pred, or a ground-truth segmentation) with the
    file's affine.  save_dir: the result is written as `<case_id>.json`.  device: a HIP device uploads the volume (as
    bytes) and measures there.  options: labels, components, min_voxels, gaps.  Prints one line per structure."""
    import nifti
    from pathlib import Path
    from utils import json_save
    pred_file = Path(pred_file)
    case_id = pred_file.name
    for suffix in ('.gz', '.nii', '.pred'):
        if case_id.endswith(suffix):
            case_id = case_id[:-len(suffix)]
    pred, affine, _ = nifti.load(pred_file)
    pred = np.ascontiguousarray(np.clip(pred, 0, 255).astype(np.uint8))
    case = {'case_id': case_id, 'affine': affine, 'pred': pred if device is None else torch.from_numpy(pred).to(device)}
    result = measure_case(case, 'pred', **options)
    for d in result['structures']:
        if d['voxels']:
            print("%s label_%s%s: %.3f ml, longest diameter %.1f mm, surface %.1f mm^2, %.0f %% exposed"
                  % (case_id, _label_name(d['label']), ' #%d' % d['component'] if 'component' in d else '',
                     d['volume_mm3'] / 1000.0, d['feret_mm'], d['surface_mm2'], 100.0 * d['exposed_fraction']))
    if save_dir is not None:
        save_dir = Path(save_dir)
        save_dir.mkdir(parents=True, exist_ok=True)
        result['file'] = str(save_dir / ('%s.json' % case_id))
        json_save(result['file'], result)
    return result


def batch_measure(pred_dir, save_dir, data_range=None, device=None, **options):
    """measure over the sorted *.nii.gz files of `pred_dir`; returns the per-file results."""
    from pathlib import Path
    pred_files = sorted(Path(pred_dir).glob('*.nii.gz'))
    return [measure(pred_files[i], save_dir, device, **options)
            for i in (data_range if data_range is not None else range(len(pred_files)))]


# ------------------------------------------------------------------ the clean-up recipe of a validation set
def _label_bytes(path, device):
    """A NIfTI label volume as contiguous uint8, numpy or uploaded to `device`."""
    import nifti
    volume, affine, _ = nifti.load(path)
    volume = np.ascontiguousarray(np.clip(volume, 0, 255).astype(np.uint8))
    return (volume if device is None else torch.from_numpy(volume).to(device)), affine


def _class_dice_means(cases, recipe, num_classes):
    """Mean over the cases of the Dice 2TP / (2TP + FP + FN) of every class 1 .. num_classes - 1 between the label and
    the prediction cleaned by `recipe`, as float64 from the integer confusion tables; a case in which a class is absent
    from both volumes does not count for that class, and a class that no case counts for has the mean None."""
    import transform
    sums = [[] for _ in range(num_classes)]
    for label, pred in cases:
        table, _ = _confusion_table({'label': label, 'pred': transform.clean_labels(pred, **recipe)})
        full = np.zeros((max(num_classes, table.shape[0]),) * 2, dtype=np.int64)
        full[:table.shape[0], :table.shape[1]] = table
        for c in range(1, num_classes):
            tp, fn, fp, _ = _class_counts(full, c)
            if tp + fn + fp:
                sums[c].append(2.0 * tp / (2.0 * tp + fp + fn))
    return [float(np.mean(np.asarray(s, dtype=np.float64))) if s else None for s in sums]


def _with_step(recipe, target, k):
    """`recipe` with the k largest components kept of `target`: 'foreground' or a class."""
    out = {key: (dict(v) if isinstance(v, dict) else v) for key, v in recipe.items()}
    if target == 'foreground':
        out['foreground'] = k
    else:
        out.setdefault('keep_largest', {})[target] = k
    return out


def determine_postprocessing(label_dir, pred_dir, num_classes=3, max_components=2, fill_holes=(), save_file=None,
                             data_range=None, device=None):
    """Which keep-the-largest-components steps help on a validation set (the rule of nnU-Net's post-processing search,
    fixed here).  The sorted *.nii.gz of `label_dir` and `pred_dir` pair up.  The targets are 'foreground' first, then
    each class 1 .. num_classes - 1 ascending, each judged on the predictions as the steps adopted so far (and the given
    `fill_holes` labels, which are applied and not searched) clean them.  For a target, k = 1 .. max_components is
    tried; a candidate's score is the mean over the affected classes (all for foreground, else the one) of the
    mean-over-cases Dice; the smallest k with the best score is adopted if that score is strictly above the score
    without the step and, for foreground, no class's mean falls below its mean without it.  Scores are float64 from
    integer tables, so device=None (scipy) and a HIP device (the kernels; only the tables come down) return the same.
    Returns {'recipe': keywords of transform.clean_labels, 'table': one entry per target}; save_file: written as JSON
    (json_save; label keys become strings there, which clean_labels accepts)."""
    from pathlib import Path
    from utils import json_save
    if num_classes < 2:
        raise ValueError("determine_postprocessing: num_classes=%r (background and at least one class)" % (num_classes,))
    if int(max_components) != max_components or not 1 <= max_components <= 8:
        raise ValueError("determine_postprocessing: max_components=%r (1 .. 8)" % (max_components,))
    label_files = sorted(Path(label_dir).glob('*.nii.gz'))
    pred_files = sorted(Path(pred_dir).glob('*.nii.gz'))
    if len(label_files) != len(pred_files):
        raise ValueError("determine_postprocessing: %d label files, %d prediction files" % (len(label_files), len(pred_files)))
    cases = [(_label_bytes(label_files[i], device)[0], _label_bytes(pred_files[i], device)[0])
             for i in (data_range if data_range is not None else range(len(label_files)))]
    if not cases:
        raise ValueError("determine_postprocessing: no case in %s" % (label_dir,))
    recipe = {'fill_holes': [int(v) for v in fill_holes]} if len(fill_holes) else {}
    table = []
    for target in ['foreground'] + list(range(1, num_classes)):
        affected = list(range(1, num_classes)) if target == 'foreground' else [target]
        base = _class_dice_means(cases, recipe, num_classes)
        scored = [c for c in affected if base[c] is not None]
        entry = {'target': target, 'class_means': base[1:], 'score': None, 'candidates': {}, 'adopted': None}
        table.append(entry)
        if not scored:                                       # no case holds an affected class: nothing to judge by
            continue
        entry['score'] = float(np.mean(np.asarray([base[c] for c in scored], dtype=np.float64)))
        best = None
        for k in range(1, int(max_components) + 1):
            means = _class_dice_means(cases, _with_step(recipe, target, k), num_classes)
            # a class that no case counts for any more (only false positives before, all removed) keeps its old mean
            after = [base[c] if means[c] is None else means[c] for c in scored]
            score = float(np.mean(np.asarray(after, dtype=np.float64)))
            harmless = all(a >= base[c] for a, c in zip(after, scored))
            entry['candidates'][k] = {'score': score, 'class_means': means[1:]}
            if best is None or score > best[1]:              # the smallest k with the best score
                best = (k, score, harmless)
        if best[1] > entry['score'] and (target != 'foreground' or best[2]):
            entry['adopted'] = best[0]
            recipe = _with_step(recipe, target, best[0])
    result = {'recipe': recipe, 'table': table}
    if save_file is not None:
        json_save(save_file, result)
    return result


def postprocess_case(case, recipe, key='pred'):
    """case[key] replaced by transform.clean_labels(case[key], **recipe), for numpy cases and cases on the device."""
    import transform
    case[key] = transform.clean_labels(case[key], **recipe)
    return case


def postprocess(pred_file, save_dir, recipe, device=None):
    """clean_labels of a NIfTI label volume (a `*.pred.nii.gz` of save_pred), written to `save_dir` as
    `<case_id>.pred.nii.gz` with the file's affine.  device: a HIP device uploads the volume and cleans it there.
    Returns the written path."""
    import nifti
    from pathlib import Path
    pred_file = Path(pred_file)
    case_id = pred_file.name
    for suffix in ('.gz', '.nii', '.pred'):
        if case_id.endswith(suffix):
            case_id = case_id[:-len(suffix)]
    pred, affine = _label_bytes(pred_file, device)
    case = postprocess_case({'case_id': case_id, 'affine': affine, 'pred': pred}, recipe)
    cleaned = case['pred'].cpu().numpy() if torch.is_tensor(case['pred']) else case['pred']
    save_dir = Path(save_dir)
    save_dir.mkdir(parents=True, exist_ok=True)
    path = save_dir / ('%s.pred.nii.gz' % case_id)
    nifti.save(cleaned.astype(np.uint8), affine, path)
    return str(path)


def batch_postprocess(pred_dir, save_dir, recipe, data_range=None, device=None):
    """postprocess over the sorted *.nii.gz files of `pred_dir`; returns the written paths."""
    from pathlib import Path
    pred_files = sorted(Path(pred_dir).glob('*.nii.gz'))
    return [postprocess(pred_files[i], save_dir, recipe, device)
            for i in (data_range if data_range is not None else range(len(pred_files)))]


# ------------------------------------------------------------------ centrelines of the tubular structures
def _ratio(num, den):
    return num / den if den else math.nan


def _radius_stats_numpy(sq):
    """skeleton.radius_stats on the host: (n, min, mean, max) of the radii whose squares are `sq`, the mean's sum in the
    order of include/ru3d.h (256 strided partial sums, then seven halving steps)."""
    n = int(sq.size)
    if not n:
        return 0, math.nan, math.nan, math.nan
    rows = np.zeros((n + 255) // 256 * 256, dtype=np.float64)
    rows[:n] = np.sqrt(sq)
    part = np.zeros(256, dtype=np.float64)
    for row in rows.reshape(-1, 256):
        part = part + row
    h = 128
    while h:
        part = part[:h] + part[h:2 * h]
        h //= 2
    return n, math.sqrt(float(sq.min())), float(part[0]) / n, math.sqrt(float(sq.max()))


def _radii_squared_numpy(skel, mask, spacing):
    """skeleton.radii_squared on the host: the squared distance from every voxel of `skel` (element order) to the nearest
    voxel outside `mask`, through scipy's feature transform and the expression the device transform is held to."""
    if mask.all():
        return np.full(int(skel.sum()), np.inf)
    return _contract_sq_numpy(skel, _nearest_feature_numpy(~mask, spacing), spacing)


def _centerline_operands(case, keys, what):
    """The volumes case[k] for k in keys on one route: uint8 HIP tensors when any of them is one, else numpy arrays
    reshaped to three axes; and the number of axes they came with."""
    volumes = [case[k] for k in keys]
    shape = tuple(volumes[0].shape)
    if any(tuple(v.shape) != shape for v in volumes):
        raise ValueError("%s: volumes of shapes %s" % (what, [tuple(v.shape) for v in volumes]))
    if not 1 <= len(shape) <= 3:
        raise ValueError("%s: a volume of shape %s (1 to 3 axes)" % (what, shape))
    hip = [v for v in volumes if _is_hip(v)]
    if hip:
        return [_device_bytes(v, hip[0].device) for v in volumes], len(shape), True
    shape3 = (1,) * (3 - len(shape)) + shape
    return [np.asarray(v.cpu() if torch.is_tensor(v) else v).reshape(shape3) for v in volumes], len(shape), False


def _packed_union(volume, values):
    import morphology
    packed = morphology.pack(volume, 'eq', values[0])
    for v in values[1:]:
        packed.bits |= morphology.pack(volume, 'eq', v).bits
    return packed


def evaluate_centerline_case(case, labels=None):
    """Centreline Dice (clDice) of every foreground class 1 .. label.max() of case['label'] vs case['pred'] (labels: a
    list of values, a tuple standing for the union of its values): a list of dicts.  With S the curve skeleton
    (transform.skeletonize) and V the mask of the class,
      tprec   |S_pred & V_label| / |S_pred|      how much of the predicted centreline lies inside the true structure,
      tsens   |S_label & V_pred| / |S_label|     how much of the true centreline the prediction covers,
      cldice  2 tprec tsens / (tprec + tsens),
    and the four integers as n_pred_skeleton, n_pred_skeleton_in_label, n_label_skeleton, n_label_skeleton_in_pred.  A
    zero denominator gives nan for that ratio.  numpy operands run on the host (the numpy twin of the thinning); when
    `pred` or `label` is a HIP tensor the other operand is uploaded and masks, skeletons (csrc/skeleton.hip) and
    counts stay on the device: per class one download of six integers beside the thinning's own iteration counter."""
    (pred, label), _, hip = _centerline_operands(case, ('pred', 'label'), "evaluate_centerline_case")
    top = 0
    if labels is None:
        top = (int(label.max().item()) if label.numel() else 0) if hip else (int(label.max()) if label.size else 0)
    results = []
    for name, values in _mesh_labels(labels, top):
        if hip:
            import skeleton
            vp, vl = _packed_union(pred, values), _packed_union(label, values)
            counts = torch.cat((skeleton.overlap_device(skeleton.thin(vp), vl),
                                skeleton.overlap_device(skeleton.thin(vl), vp))).tolist()
            sp, sp_in, sl, sl_in = int(counts[0]), int(counts[2]), int(counts[3]), int(counts[5])
        else:
            import transform
            vp, vl = np.isin(pred, values), np.isin(label, values)
            s_pred, s_label = transform._skeleton_numpy(vp)[0], transform._skeleton_numpy(vl)[0]
            sp, sp_in, sl, sl_in = int(s_pred.sum()), int((s_pred & vl).sum()), int(s_label.sum()), int((s_label & vp).sum())
        tprec, tsens = _ratio(sp_in, sp), _ratio(sl_in, sl)
        both = tprec + tsens
        results.append({'label': name, 'tprec': tprec, 'tsens': tsens,
                        'cldice': 2 * tprec * tsens / both if both > 0 else math.nan,
                        'n_pred_skeleton': sp, 'n_pred_skeleton_in_label': sp_in,
                        'n_label_skeleton': sl, 'n_label_skeleton_in_pred': sl_in})
    return results


def evaluate_centerline(label_file, pred_file, device=None):
    """evaluate_centerline_case of two NIfTI files.  device: a HIP device uploads both volumes (as bytes) and evaluates
    there."""
    import nifti
    label, _, _ = nifti.load(label_file)
    pred, _, _ = nifti.load(pred_file)
    case = {'label': label.astype(np.uint8), 'pred': pred.astype(np.uint8)}
    if device is not None:
        case = {k: torch.from_numpy(np.ascontiguousarray(v)).to(device) for k, v in case.items()}
    return evaluate_centerline_case(case)


def batch_evaluate_centerline(label_dir, pred_dir, data_range=None, device=None):
    """evaluate_centerline over the sorted *.nii.gz files of two directories; prints the mean of each ratio per class
    (over the cases that have the class and a defined ratio) and returns the per-case lists."""
    from pathlib import Path
    label_files = sorted(Path(label_dir).glob('*.nii.gz'))
    pred_files = sorted(Path(pred_dir).glob('*.nii.gz'))
    results = [evaluate_centerline(label_files[i], pred_files[i], device)
               for i in (data_range if data_range is not None else range(len(label_files)))]
    for key in ('cldice', 'tprec', 'tsens'):
        print('\nThe mean %s of each label:' % key)
        for c in range(max((len(r) for r in results), default=0)):
            values = [r[c][key] for r in results if len(r) > c and not math.isnan(r[c][key])]
            print("label_%d: %f" % (c + 1, np.mean(values) if values else math.nan))
    return results


def centerline_case(case, labels=None, key='pred', return_device=False):
    """The centreline of every structure of the label volume `case[key]`: a list of dicts
      label       the value (or the tuple of values whose union was thinned),
      voxels, ends, junctions   the skeleton's voxel count, its end voxels (one neighbour among the 26) and its
                  junction voxels (three or more),
      length      of the skeleton's voxel graph in millimetres (skeleton.length: every pair of 26-adjacent voxels counts),
      radius_min, radius_mean, radius_max   distance from the skeleton voxels to the nearest voxel outside the structure,
      points, radii   float64 [n, 3] world coordinates (`case['affine']`; voxel coordinates without one) of the skeleton
                  voxels in element order and float64 [n] radii - left out with return_device=True.
    The voxel spacing is that of the affine.  A numpy volume takes the numpy route; a HIP volume is packed, thinned,
    classified and measured on the device (csrc/skeleton.hip, csrc/distance.hip) and only the numbers above, or with
    return_device=False the points and radii too, are downloaded."""
    from data import get_spacing
    import transform
    (volume,), ndim, hip = _centerline_operands(case, (key,), "centerline_case")
    affine = np.asarray(case['affine'], dtype=np.float64) if case.get('affine') is not None else np.eye(4)
    spacing = get_spacing(affine)
    top = 0
    if labels is None:
        top = (int(volume.max().item()) if volume.numel() else 0) if hip else (int(volume.max()) if volume.size else 0)
    results = []
    for name, values in _mesh_labels(labels, top):
        if hip:
            import mesh
            import morphology
            import skeleton
            mask = _packed_union(volume, values)
            skel = skeleton.thin(mask)
            _, _, n, n_ends, n_junctions = skeleton.classify(skel)
            total = skeleton.length(skel, spacing[3 - ndim:])
            sq = skeleton.radii_squared(skel, mask, spacing[3 - ndim:])
            _, lo, mean, hi = skeleton.radius_stats(sq)
            if not return_device:
                index = torch.nonzero(morphology.unpack(skel).reshape(skel.shape3)).to(torch.float64)
                points = mesh.to_world(index, affine).cpu().numpy()
                radii = np.sqrt(sq.cpu().numpy())
        else:
            mask = np.isin(volume, values)
            skel = transform._skeleton_numpy(mask)[0]
            _, _, n, n_ends, n_junctions = transform._skeleton_classify_numpy(skel)
            total = transform._skeleton_length_numpy(skel, spacing)
            sq = _radii_squared_numpy(skel, mask, spacing)
            _, lo, mean, hi = _radius_stats_numpy(sq)
            points = transform._to_world_numpy(np.argwhere(skel).astype(np.float64), np.zeros((0, 3), np.int32), affine)[0]
            radii = np.sqrt(sq)
        result = {'label': name, 'voxels': n, 'ends': n_ends, 'junctions': n_junctions, 'length': total,
                  'radius_min': lo, 'radius_mean': mean, 'radius_max': hi}
        if not return_device:
            result.update(points=points, radii=radii)
        results.append(result)
    return results


def extract_centerline(pred_file, save_dir=None, device=None, labels=None):
    """centerline_case of a NIfTI label volume with the file's affine.  save_dir: every non-empty centreline is written as
    `<case_id>.label_<n>.centerline.ply`, a vertex-only binary PLY with x, y, z and radius per skeleton voxel
    (meshfile.write_points_ply), and its dict gains 'file'.  device: a HIP device uploads the volume (as bytes) and works
    there.  Prints one line per structure; returns the list of dicts."""
    import nifti
    import meshfile
    from pathlib import Path
    pred_file = Path(pred_file)
    case_id = pred_file.name
    for suffix in ('.gz', '.nii', '.pred'):
        if case_id.endswith(suffix):
            case_id = case_id[:-len(suffix)]
    pred, affine, _ = nifti.load(pred_file)
    pred = np.ascontiguousarray(np.clip(pred, 0, 255).astype(np.uint8))
    case = {'case_id': case_id, 'affine': affine, 'pred': pred if device is None else torch.from_numpy(pred).to(device)}
    results = centerline_case(case, labels, 'pred')
    if save_dir is not None:
        save_dir = Path(save_dir)
        save_dir.mkdir(parents=True, exist_ok=True)
    for r in results:
        print("%s label_%s: %d centreline voxels, %d ends, %d junctions, length %.1f mm, radius %.2f / %.2f / %.2f mm"
              % (case_id, _label_name(r['label']), r['voxels'], r['ends'], r['junctions'], r['length'], r['radius_min'],
                 r['radius_mean'], r['radius_max']))
        if save_dir is not None and r['voxels']:
            r['file'] = save_dir / ('%s.label_%s.centerline.ply' % (case_id, _label_name(r['label'])))
            meshfile.write_points_ply(r['file'], r['points'], r['radii'])
    return results


def batch_extract_centerline(pred_dir, save_dir, data_range=None, device=None, labels=None):
    """extract_centerline over the sorted *.nii.gz files of `pred_dir`; returns the per-file lists."""
    from pathlib import Path
    pred_files = sorted(Path(pred_dir).glob('*.nii.gz'))
    return [extract_centerline(pred_files[i], save_dir, device, labels)
            for i in (data_range if data_range is not None else range(len(pred_files)))]


# ------------------------------------------------------------------ vessel trees: nodes and branches of a centreline
def _vessel_graph_dict(name, g, rounds, affine):
    """The graph `g` (skeleton.graph or its numpy twin, with radii) of one structure as plain Python numbers and lists."""
    import transform
    nodes, branches = g['node_table'], g['branch_table']
    centroids = nodes[:, 2:5].astype(np.float64) / nodes[:, 0:1].astype(np.float64)
    world = transform._to_world_numpy(centroids, np.zeros((0, 3), np.int32), affine)[0]
    segments = []
    for b in range(g['branches']):
        segments.append({'id': b + 1, 'nodes': [int(branches[b, 3]), int(branches[b, 4])], 'voxels': int(branches[b, 0]),
                         'length': float(g['length'][b]), 'chord': float(g['chord'][b]),
                         'tortuosity': float(g['tortuosity'][b]), 'radius_min': float(g['radius_min'][b]),
                         'radius_mean': float(g['radius_mean'][b]), 'radius_max': float(g['radius_max'][b])})
    return {'label': name, 'nodes': g['nodes'], 'branches': g['branches'],
            'bifurcations': int((nodes[:, 1] >= 3).sum()), 'endpoints': int((nodes[:, 1] == 1).sum()),
            'loops': int((branches[:, 3] < 0).sum()), 'pruned_rounds': rounds, 'segments': segments,
            'node_centroids': [[float(v) for v in p] for p in world]}


def vessel_graph_case(case, labels=None, key='pred', min_branch_mm=0.0):
    """The vessel tree of every structure of the label volume `case[key]` as a graph: the structure is thinned
    (transform.skeletonize), spurs shorter than min_branch_mm are pruned (skeleton.prune; 0 prunes nothing), and the
    skeleton's voxel graph is read as nodes and branches (skeleton.graph, include/ru3d.h "skeleton graph").  A list of
    dicts of plain numbers and lists, ready for json:
      label           the value (or the tuple of values whose union was thinned),
      nodes, branches   their numbers; bifurcations (nodes of valence >= 3), endpoints (valence 1), loops (closed
                      branches without a node), pruned_rounds (rounds of pruning run, 0 without pruning),
      segments        per branch: id, nodes (the two it hangs on, -1 -1 for a loop), voxels, length, chord and radius_min /
                      radius_mean / radius_max in millimetres, tortuosity = length / chord,
      node_centroids  per node, world coordinates (`case['affine']`; voxel coordinates without one).
    The voxel spacing is that of the affine.  A numpy volume takes the numpy route (the twins in transform.py); a HIP
    volume is packed, thinned, pruned and labelled on the device (csrc/skeleton.hip, csrc/skeleton_graph.hip) and only
    the tables come down.  Both routes give the same numbers."""
    from data import get_spacing
    import transform
    (volume,), ndim, hip = _centerline_operands(case, (key,), "vessel_graph_case")
    if not float(min_branch_mm) >= 0:
        raise ValueError("vessel_graph_case: min_branch_mm=%r (>= 0)" % (min_branch_mm,))
    affine = np.asarray(case['affine'], dtype=np.float64) if case.get('affine') is not None else np.eye(4)
    spacing = get_spacing(affine)
    top = 0
    if labels is None:
        top = (int(volume.max().item()) if volume.numel() else 0) if hip else (int(volume.max()) if volume.size else 0)
    results = []
    for name, values in _mesh_labels(labels, top):
        rounds = 0
        if hip:
            import skeleton
            mask = _packed_union(volume, values)
            skel = skeleton.thin(mask)
            if min_branch_mm > 0:
                skel, rounds = skeleton.prune(skel, min_branch_mm, spacing[3 - ndim:])
            g = skeleton.graph(skel, mask, spacing[3 - ndim:])
        else:
            mask = np.isin(volume, values)
            skel = transform._skeleton_numpy(mask)[0]
            if min_branch_mm > 0:
                skel, rounds = transform._skeleton_prune_numpy(skel, min_branch_mm, spacing)
            g = transform._skeleton_graph_numpy(skel, _radii_squared_numpy(skel, mask, spacing), spacing)
        results.append(_vessel_graph_dict(name, g, rounds, affine))
    return results


def extract_vessel_graph(pred_file, save_dir=None, device=None, labels=None, min_branch_mm=0.0):
    """vessel_graph_case of a NIfTI label volume with the file's affine.  save_dir: every structure's graph is written as
    `<case_id>.label_<n>.graph.json` (utils.json_save) and its dict gains 'file'.  device: a HIP device uploads the volume
    (as bytes) and works there.  Prints one line per structure; returns the list of dicts."""
    import nifti
    from pathlib import Path
    from utils import json_save
    pred_file = Path(pred_file)
    case_id = pred_file.name
    for suffix in ('.gz', '.nii', '.pred'):
        if case_id.endswith(suffix):
            case_id = case_id[:-len(suffix)]
    pred, affine, _ = nifti.load(pred_file)
    pred = np.ascontiguousarray(np.clip(pred, 0, 255).astype(np.uint8))
    case = {'case_id': case_id, 'affine': affine, 'pred': pred if device is None else torch.from_numpy(pred).to(device)}
    results = vessel_graph_case(case, labels, 'pred', min_branch_mm)
    if save_dir is not None:
        save_dir = Path(save_dir)
        save_dir.mkdir(parents=True, exist_ok=True)
    for r in results:
        print("%s label_%s: %d nodes (%d bifurcations, %d endpoints), %d branches (%d loops), %.1f mm of branches, "
              "%d pruning rounds" % (case_id, _label_name(r['label']), r['nodes'], r['bifurcations'], r['endpoints'],
                                     r['branches'], r['loops'], sum(s['length'] for s in r['segments']), r['pruned_rounds']))
        if save_dir is not None:
            path = save_dir / ('%s.label_%s.graph.json' % (case_id, _label_name(r['label'])))
            json_save(path, r)
            r['file'] = path
    return results


# ------------------------------------------------------------------ vessel territories: an organ by nearest branch
def _label_values(entry, what):
    values = tuple(int(v) for v in entry) if isinstance(entry, (tuple, list)) else (int(entry),)
    if not values or any(v < 1 or v > 255 for v in values):
        raise ValueError("vessel_territories_case: %s=%r (a value 1 .. 255, or a tuple of them)" % (what, entry))
    return values


def vessel_territories_case(case, vessel, organ, other=None, key='pred', min_branch_mm=0.0, root=None,
                            return_labels=False, metric='euclidean'):
    """Which part of an organ every branch of a vessel tree feeds: the structure `vessel` of the label volume
    `case[key]` is thinned, pruned and read as a graph exactly as vessel_graph_case does, and the voxels of `organ` -
    together with those of `other` (a tumour is part of the organ it grows in, though it has a label of its own) - are
    partitioned by their nearest centreline voxel under the affine's spacing (territory.nearest: the exact Euclidean
    feature transform, ties by the rule of include/ru3d.h).  vessel, organ, other: a label value or a tuple of values.
    With organ == vessel every vessel voxel gets its branch: the vessel mask coloured by branch, and the territories are
    the branches' vessel volumes.  metric='geodesic' measures along a path instead of a straight line: the centreline
    voxels, each carrying its branch's or node's id, are grown through the region united with the vessel mask over the
    26 neighbour steps (geodesic.grow, include/ru3d.h "geodesic distance"), so parenchyma across the renal sinus, a cyst
    or a gap falls to the branch that reaches it through tissue, a lumen voxel to a branch of its own vessel, and a
    region voxel that no path reaches is unassigned.  Returns the dict of vessel_graph_case for the vessel, with, per segment,
      territory_voxels, territory_ml   the voxels nearest to the branch's own path voxels, and their volume,
      downstream_voxels, downstream_ml   the same for the branch, the node it leads to and everything beyond it in the
                      tree rooted at `root` (territory.rooted: None picks the end node whose branch is thickest, the
                      ostium; else a node number),
      parent, depth, order, reachable, chord   the branch's place in that tree (order: Strahler's),
      other_voxels, downstream_other_voxels, downstream_other_fraction   with `other`: its voxels in the territory, in
                      everything downstream, and the share of all of `other` that the branch and its subtree supply,
    and root, organ_voxels (the partitioned voxels), unassigned_voxels (those of a case without any centreline),
    node_territory_voxels (per node; they go downstream with the branch that reaches the node) and, with `other`,
    other_voxels.  return_labels=True adds 'labels', the int32 volume of territories (branch b -> b, node m ->
    branches + m, 0 outside the organ), a HIP tensor on the device route.  numpy volumes take the twins of transform.py;
    a HIP volume stays on the device (csrc/skeleton.hip, csrc/skeleton_graph.hip, csrc/territory.hip) and only the
    graph's tables and the tally come down.  Both routes give the same numbers."""
    from data import get_spacing
    import territory
    import transform
    (volume,), ndim, hip = _centerline_operands(case, (key,), "vessel_territories_case")
    if not float(min_branch_mm) >= 0:
        raise ValueError("vessel_territories_case: min_branch_mm=%r (>= 0)" % (min_branch_mm,))
    vessel_values, organ_values = _label_values(vessel, 'vessel'), _label_values(organ, 'organ')
    other_values = _label_values(other, 'other') if other is not None else ()
    region_values = tuple(sorted(set(organ_values) | set(other_values)))
    affine = np.asarray(case['affine'], dtype=np.float64) if case.get('affine') is not None else np.eye(4)
    spacing = get_spacing(affine)
    territory.check_metric(metric, "vessel_territories_case")
    rounds = 0
    if hip:
        import morphology
        import skeleton
        mask = _packed_union(volume, vessel_values)
        skel = skeleton.thin(mask)
        if min_branch_mm > 0:
            skel, rounds = skeleton.prune(skel, min_branch_mm, spacing[3 - ndim:])
        g = skeleton.graph(skel, mask, spacing[3 - ndim:])
        tumour = morphology.unpack(_packed_union(volume, other_values)) if other_values else None
        table, labels = territory.partition(skel, g, _packed_union(volume, region_values), spacing[3 - ndim:], tumour,
                                            1 if other_values else 0, metric, mask)
    else:
        mask = np.isin(volume, vessel_values)
        skel = transform._skeleton_numpy(mask)[0]
        if min_branch_mm > 0:
            skel, rounds = transform._skeleton_prune_numpy(skel, min_branch_mm, spacing)
        g = transform._skeleton_graph_numpy(skel, _radii_squared_numpy(skel, mask, spacing), spacing)
        region = np.isin(volume, region_values)
        tumour = np.isin(volume, other_values).astype(np.uint8) if other_values else None
        site_ids, K = territory.branch_sites(g)
        if metric == 'geodesic':
            import geodesic
            seeds = np.zeros(skel.shape, dtype=np.int32)
            seeds[skel] = site_ids
            weights = geodesic.step_weights(spacing[3 - ndim:], ndim, 3)
            labels = np.where(region, transform._geodesic_numpy(seeds, region | mask, weights, geodesic.UNLIMITED)[1], 0)
            labels = labels.astype(np.int32)
        else:
            index, _ = transform._nearest_site_numpy(skel, spacing)
            labels = transform._site_assign_numpy(skel, site_ids, index, region)
        table = transform._territory_tally_numpy(labels, K, tumour, 1 if other_values else 0, region)
        labels = labels.reshape(tuple(case[key].shape))
    B = g['branches']
    tree = territory.rooted(g['node_table'], g['branch_table'], g['radius_mean'], root)
    down = territory.downstream(table, tree, B)
    voxel_ml = float(spacing[0] * spacing[1] * spacing[2]) / 1000.0
    other_total = int(table[:, 1].sum()) if other_values else 0
    result = _vessel_graph_dict(vessel_values if isinstance(vessel, (tuple, list)) else int(vessel), g, rounds, affine)
    for b, s in enumerate(result['segments']):
        own, below = int(table[b + 1].sum()), int(down[b].sum())
        s.update(territory_voxels=own, territory_ml=own * voxel_ml, downstream_voxels=below, downstream_ml=below * voxel_ml,
                 parent=int(tree['parent'][b]), depth=int(tree['depth'][b]), order=int(tree['order'][b]),
                 reachable=bool(tree['reachable'][b]), chord=bool(tree['chord'][b]))
        if other_values:
            s.update(other_voxels=int(table[b + 1, 1]), downstream_other_voxels=int(down[b, 1]),
                     downstream_other_fraction=_ratio(int(down[b, 1]), other_total))
    result.update(root=int(tree['root']), organ_voxels=int(table.sum()), unassigned_voxels=int(table[0].sum()),
                  node_territory_voxels=[int(v) for v in table[B + 1:].sum(axis=1)])
    if other_values:
        result['other_voxels'] = other_total
    if return_labels:
        result['labels'] = labels
    return result


def extract_vessel_territories(pred_file, save_dir=None, device=None, vessel=None, organ=None, other=None,
                               min_branch_mm=0.0, root=None, metric='euclidean'):
    """vessel_territories_case of a NIfTI label volume with the file's affine (vessel and organ are required; organ ==
    vessel colours the vessel mask by branch).  save_dir: the dict is written as `<case_id>.label_<n>.territories.json`
    (n names the vessel; utils.json_save) and the int32 volume of territories as `<case_id>.label_<n>.territories.nii.gz`
    with the file's affine; the dict gains 'file' and 'labels_file'.  metric: 'euclidean' or 'geodesic', as there.
    device: a HIP device uploads the volume (as bytes) and works there; the label volume is the one download beside the
    tables.  Prints one line; returns the dict."""
    import nifti
    from pathlib import Path
    from utils import json_save
    if vessel is None or organ is None:
        raise ValueError("extract_vessel_territories: vessel and organ are required (label values or tuples of values)")
    pred_file = Path(pred_file)
    case_id = pred_file.name
    for suffix in ('.gz', '.nii', '.pred'):
        if case_id.endswith(suffix):
            case_id = case_id[:-len(suffix)]
    pred, affine, _ = nifti.load(pred_file)
    pred = np.ascontiguousarray(np.clip(pred, 0, 255).astype(np.uint8))
    case = {'case_id': case_id, 'affine': affine, 'pred': pred if device is None else torch.from_numpy(pred).to(device)}
    r = vessel_territories_case(case, vessel, organ, other, 'pred', min_branch_mm, root, return_labels=True, metric=metric)
    labels = r.pop('labels')
    fed = [s['downstream_ml'] for s in r['segments'] if s['reachable'] and not s['chord'] and s['parent'] == 0]
    print("%s label_%s: %d branches from node %d, %d organ voxels in territories (%d unassigned), %.1f ml below the root"
          % (case_id, _label_name(r['label']), r['branches'], r['root'], r['organ_voxels'] - r['unassigned_voxels'],
             r['unassigned_voxels'], sum(fed))
          + (", %d voxels of label_%s" % (r['other_voxels'], '_'.join(str(v) for v in _label_values(other, 'other')))
             if other is not None else ""))
    if save_dir is not None:
        save_dir = Path(save_dir)
        save_dir.mkdir(parents=True, exist_ok=True)
        stem = '%s.label_%s.territories' % (case_id, _label_name(r['label']))
        json_save(save_dir / (stem + '.json'), r)
        nifti.save(labels.cpu().numpy() if torch.is_tensor(labels) else labels, affine, save_dir / (stem + '.nii.gz'))
        r['file'], r['labels_file'] = save_dir / (stem + '.json'), save_dir / (stem + '.nii.gz')
    return r


def batch_extract_vessel_territories(pred_dir, save_dir, data_range=None, device=None, **options):
    """extract_vessel_territories over the sorted *.nii.gz files of `pred_dir`; returns the per-file dicts."""
    from pathlib import Path
    pred_files = sorted(Path(pred_dir).glob('*.nii.gz'))
    return [extract_vessel_territories(pred_files[i], save_dir, device, **options)
            for i in (data_range if data_range is not None else range(len(pred_files)))]


# ------------------------------------------------------------------ local thickness: calibre and parenchyma thickness
THICKNESS_Q = (5.0, 50.0, 95.0)


def _thickness_stats_numpy(t2_values, q=THICKNESS_Q):
    """thickness.summary on the host: the same dict from the float64 vector of T2 over a structure's voxels."""
    n = int(t2_values.size)
    if n == 0:
        return {'n': 0}
    ordered = np.sort(t2_values)
    thick = 2.0 * np.sqrt(ordered)
    return {'n': n, 't2_max': float(ordered[-1]), 't2_min': float(ordered[0]),
            'order': {float(v): tuple(float(ordered[r]) for r in _percentile_ranks(n, float(v))) for v in q},
            'mean': float(thick.mean()), 'std': float(thick.std())}


def _thickness_metrics(stats):
    """voxels, min, mean, std, max and the percentiles p05 .. of the thickness from the dict of thickness.summary (or its
    host twin).  The square roots are taken here, on a handful of numbers; a percentile is np.percentile's linear
    interpolation between the roots of its two order statistics, written out as in _surface_metrics."""
    n = stats['n']
    if n == 0:
        return {'voxels': 0}
    out = {'voxels': n, 'min': 2.0 * math.sqrt(stats['t2_min']), 'mean': stats['mean'], 'std': stats['std'],
           'max': 2.0 * math.sqrt(stats['t2_max'])}
    for v, (lo, hi) in stats['order'].items():
        lo, hi = 2.0 * math.sqrt(lo), 2.0 * math.sqrt(hi)
        gamma = v / 100.0 * (n - 1) - _percentile_ranks(n, v)[0]
        if lo == hi:
            value = lo                                  # also the full mask, where both are inf
        else:
            value = hi - (hi - lo) * (1 - gamma) if gamma >= 0.5 else lo + (hi - lo) * gamma
        out['p%02d' % int(round(v))] = value
    return out


def thickness_case(case, labels=None, key='pred', return_device=False, return_map=False):
    """The local thickness of every structure of the label volume `case[key]` (include/ru3d.h, "local thickness"): per
    voxel the diameter of the largest ball that fits inside the structure and contains the voxel - the calibre of a
    vessel at every lumen voxel, the thickness of the parenchyma.  A list of dicts of plain numbers, ready for json:
      label     the value (or the tuple of values whose union was measured),
      voxels    the structure's voxels (an empty structure has this entry alone),
      min, mean, std, max, p05, p50, p95   of the thickness over those voxels, in millimetres (std: population).
    The voxel spacing is that of the affine (`case['affine']`; 1 without one); distances run between voxel centres.
    return_map=True returns (list, map): the float32 volume of the thickness in millimetres, every voxel carrying the
    thickness of its own label's structure (the later entry where entries overlap), 0 in the background - a HIP tensor
    with return_device on the device route, else numpy.  A numpy volume takes the numpy route
    (transform._local_thickness_numpy, quadratic in a structure's voxels); a HIP volume is packed and measured on the
    device (csrc/thickness.hip) and one vector of numbers per structure comes down.  Both routes give the same numbers:
    the order statistics exactly, mean and std to summation order.  A structure that fills its volume has no clear voxel to
    measure against: every figure is inf and std is nan (json writes Infinity and NaN)."""
    from data import get_spacing
    import transform
    (volume,), ndim, hip = _centerline_operands(case, (key,), "thickness_case")
    affine = np.asarray(case['affine'], dtype=np.float64) if case.get('affine') is not None else np.eye(4)
    spacing = tuple(float(v) for v in get_spacing(affine))
    top = 0
    if labels is None:
        top = (int(volume.max().item()) if volume.numel() else 0) if hip else (int(volume.max()) if volume.size else 0)
    shape = tuple(case[key].shape)
    results, tmap = [], None
    if return_map:
        tmap = torch.zeros(shape, dtype=torch.float32, device=volume.device) if hip else np.zeros(shape, dtype=np.float32)
    for name, values in _mesh_labels(labels, top):
        if hip:
            import thickness
            mask = _packed_union(volume, values)
            t2 = thickness.local_squared(mask, spacing[3 - ndim:])
            stats = thickness.summary(t2, mask, THICKNESS_Q)
            if return_map and stats['n']:
                tmap = torch.where(t2 > 0, thickness.diameter(t2).to(torch.float32), tmap)
        else:
            mask = np.isin(volume, values)
            t2 = transform._local_thickness_numpy(mask, spacing)
            stats = _thickness_stats_numpy(t2[mask], THICKNESS_Q)
            if return_map and stats['n']:
                tmap = np.where(mask, (2.0 * np.sqrt(t2)).astype(np.float32), tmap.reshape(mask.shape)).reshape(shape)
        results.append(dict(label=name, **_thickness_metrics(stats)))
    if not return_map:
        return results
    if hip and not return_device:
        tmap = tmap.cpu().numpy()
    return results, tmap


def measure_thickness(pred_file, save_dir=None, device=None, labels=None, save_map=True):
    """thickness_case of a NIfTI label volume with the file's affine.  save_dir: every structure's numbers are written as
    `<case_id>.label_<n>.thickness.json` (utils.json_save; the dict gains 'file') and, with save_map, the float32 map of
    the thickness in millimetres as `<case_id>.thickness.nii.gz` with the file's affine.  device: a HIP device uploads the
    volume (as bytes) and works there; the map is the one large download.  Prints one line per structure; returns the
    list of dicts."""
    import nifti
    from pathlib import Path
    from utils import json_save
    pred_file = Path(pred_file)
    case_id = pred_file.name
    for suffix in ('.gz', '.nii', '.pred'):
        if case_id.endswith(suffix):
            case_id = case_id[:-len(suffix)]
    pred, affine, _ = nifti.load(pred_file)
    pred = np.ascontiguousarray(np.clip(pred, 0, 255).astype(np.uint8))
    case = {'case_id': case_id, 'affine': affine, 'pred': pred if device is None else torch.from_numpy(pred).to(device)}
    want_map = bool(save_map) and save_dir is not None
    results = thickness_case(case, labels, 'pred', return_map=want_map)
    tmap = None
    if want_map:
        results, tmap = results
    if save_dir is not None:
        save_dir = Path(save_dir)
        save_dir.mkdir(parents=True, exist_ok=True)
    for r in results:
        if r['voxels']:
            print("%s label_%s: %d voxels, thickness %.2f mm (median %.2f, p05 %.2f, p95 %.2f, max %.2f)"
                  % (case_id, _label_name(r['label']), r['voxels'], r['mean'], r['p50'], r['p05'], r['p95'], r['max']))
        else:
            print("%s label_%s: empty" % (case_id, _label_name(r['label'])))
        if save_dir is not None:
            path = save_dir / ('%s.label_%s.thickness.json' % (case_id, _label_name(r['label'])))
            json_save(path, r)
            r['file'] = path
    if tmap is not None:
        nifti.save(tmap, affine, save_dir / ('%s.thickness.nii.gz' % case_id))
    return results


def batch_measure_thickness(pred_dir, save_dir, data_range=None, device=None, **options):
    """measure_thickness over the sorted *.nii.gz files of `pred_dir`; returns the per-file lists."""
    from pathlib import Path
    pred_files = sorted(Path(pred_dir).glob('*.nii.gz'))
    return [measure_thickness(pred_files[i], save_dir, device, **options)
            for i in (data_range if data_range is not None else range(len(pred_files)))]


def preview_case(case, key='pred', axes=(0, 1, 2), num_slices=8, views=((30, 20), (120, 20), (210, -20)), size=256,
                 alpha=None, labels=None, colours=None, window=None, pixel_mm=None):
    """One picture of a case to leaf through, uint8 [H, W, 3]: `visualize.case_sheet` (slices of the image under the
    filled label and the outlined prediction; without an image the mask alone) and below it the shaded views of
    `visualize.render_case` of case[key], side by side.  alpha=None makes label 1 translucent (0.35) when the volume may
    hold more than one label, so that what lies inside the kidney shows.  numpy volumes take the numpy route, HIP
    tensors - for instance what `cascade_predict_case(..., return_device=True)` returns - are rendered on the device
    (csrc/render.hip) and only the pictures are downloaded."""
    import visualize
    overlays = tuple(k for k in ('label', 'pred') if case.get(k) is not None)
    if key not in case or case[key] is None:
        raise ValueError("preview_case: the case has no %r" % (key,))
    sheet = visualize.case_sheet(case, axes, num_slices, window, overlays, pixel_mm, colours)
    if alpha is None:
        alpha = {1: 0.35} if labels is None or len(tuple(labels)) > 1 else 1.0
    shots = visualize.render_case(case, key, labels, views, size, alpha, colours) if len(views) else ()
    gap = 2
    width = max(sheet.shape[1], len(shots) * (size + gap) - gap)
    out = np.zeros((sheet.shape[0] + ((gap + size) if len(shots) else 0), width, 3), dtype=np.uint8)
    out[:sheet.shape[0], :sheet.shape[1]] = sheet
    for i, shot in enumerate(shots):
        out[sheet.shape[0] + gap:, i * (size + gap):i * (size + gap) + size] = shot
    return out


def preview(pred_file, image_file=None, label_file=None, save_dir=None, device=None, **options):
    """preview_case of a NIfTI label volume (a `*.pred.nii.gz` of save_pred) with the file's affine, over the image and
    beside the ground truth when their files are given.  save_dir: the picture is written as `<case_id>.preview.png`
    (pngfile.write_png).  device: a HIP device uploads the volumes once and renders there.  `options` go to
    preview_case.  Returns the picture."""
    import nifti
    import pngfile
    from pathlib import Path
    pred_file = Path(pred_file)
    case_id = pred_file.name
    for suffix in ('.gz', '.nii', '.pred'):
        if case_id.endswith(suffix):
            case_id = case_id[:-len(suffix)]
    pred, affine, _ = nifti.load(pred_file)
    case = {'case_id': case_id, 'affine': affine, 'pred': np.ascontiguousarray(np.clip(pred, 0, 255).astype(np.uint8))}
    if label_file is not None:
        case['label'] = np.ascontiguousarray(np.clip(nifti.load(label_file)[0], 0, 255).astype(np.uint8))
    if image_file is not None:
        image = np.asarray(nifti.load(image_file)[0], dtype=np.float32)
        case['image'] = np.ascontiguousarray(image[..., None] if image.ndim == 3 else image)
    if device is not None:
        for k in ('pred', 'label', 'image'):
            if k in case:
                case[k] = torch.from_numpy(case[k]).to(device)
    picture = preview_case(case, **options)
    if save_dir is not None:
        save_dir = Path(save_dir)
        save_dir.mkdir(parents=True, exist_ok=True)
        pngfile.write_png(save_dir / ('%s.preview.png' % case_id), picture)
    return picture


def batch_preview(pred_dir, save_dir, image_dir=None, label_dir=None, data_range=None, device=None, **options):
    """preview over the sorted *.nii.gz files of `pred_dir`, one PNG per case in `save_dir`; the i-th sorted file of
    `image_dir` / `label_dir` belongs to the i-th prediction, as in batch_evaluate.  Returns the pictures."""
    from pathlib import Path
    pred_files = sorted(Path(pred_dir).glob('*.nii.gz'))
    image_files = sorted(Path(image_dir).glob('*.nii.gz')) if image_dir is not None else None
    label_files = sorted(Path(label_dir).glob('*.nii.gz')) if label_dir is not None else None
    for name, files in (('image_dir', image_files), ('label_dir', label_files)):
        if files is not None and len(files) != len(pred_files):
            raise ValueError("batch_preview: %d files in %s for %d predictions" % (len(files), name, len(pred_files)))
    return [preview(pred_files[i], image_files[i] if image_files else None, label_files[i] if label_files else None,
                    save_dir, device, **options)
            for i in (data_range if data_range is not None else range(len(pred_files)))]
