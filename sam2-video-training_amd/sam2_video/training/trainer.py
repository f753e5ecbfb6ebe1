"""SAM2LightningModule / SAM2LightningDataModule drop-ins (reference
sam2_video/training/trainer.py:28-400) and a Lightning-API Trainer for them.

* `SAM2LightningModule(model, loss, optimizer, scheduler, visualization)`: same
  constructor sections, loss selection (multi_step | bce), gt_stride,
  training_step / validation_step signatures and logged keys.  It subclasses
  `lightning.pytorch.LightningModule` when Lightning is importable, else
  `nn.Module`.  `configure_optimizers` returns the arena AdamW (eps/amsgrad of
  the YAML are ignored exactly as the reference does, trainer.py:124-130) with
  the cosine-with-warmup schedule stepped per optimizer step.
* `SAM2LightningDataModule(data, train_shuffle)`: DataLoaders of B == 1 clips
  collated by `sam2_collate_fn` (trainer.py:325-400); COCO files when the data
  section's paths exist, synthetic clips of the data section's shape otherwise.
* `Trainer(**cfg.trainer)`: the `lightning.pytorch.Trainer` arguments the
  reference configs set (best.yaml:98-113) -- max_epochs / max_steps,
  accumulate_grad_batches, gradient_clip_val (0 / None = no clip, as Lightning),
  precision, val_check_interval, num_sanity_val_steps, limit_*_batches,
  callbacks, default_root_dir -- and `fit(module, datamodule)`.  `model/build.py`
  resolves the configs' `_target_: lightning.pytorch.trainer.trainer.Trainer` to
  it when Lightning is not installed (it is not in this image).  `callbacks`
  (training/callbacks.py: ModelCheckpoint, EarlyStopping,
  StochasticWeightAveraging, ...) get on_fit_start, on_train_epoch_start,
  on_validation_end (after every validation but the sanity one),
  on_train_epoch_end and on_train_end; `callback_metrics`, `should_stop`,
  `checkpoint_callback` and `early_stopping_callback` are Lightning's attributes.
  `fit(..., ckpt_path=PATH)` continues the run a checkpoint of `save_checkpoint` was taken from, bit for bit
  (training/resume.py); a Lightning / reference checkpoint restores weights, optimizer state,
  global_step and epoch.
* `StepRunner`: one micro-step of the fit loop on the device (captured HIP
  graph per input signature), RCCL all-reduce + clip + AdamW at accumulation
  boundaries.

* Visualisation (reference trainer.py:206-252 `_should_log_gif` / `_log_gif`): the reference's schedule
  (`visualization.enabled`, `train_every_n_steps`, `val_first_batch_every_n_epochs`, `max_length`, `stride`,
  `caption`) with a file sink instead of W&B: when the new key `visualization.save_dir` is set (default null:
  nothing is rendered) a scheduled step composes the 2 x 2 frames on the device (utils/viz.py) and writes
  `<save_dir>/{split}_e{epoch:04d}_s{global_step:07d}.gif` with Pillow.  Under StepRunner graphs the hook runs
  after the replay, outside every capture, on the static batch, `last_outputs` and the prompt plan's host points;
  it synchronises on the steps it fires and on no other.

The reference's per-step torch.cuda.synchronize() + empty_cache()
(trainer.py:186-187) are host syncs with no effect on results and are omitted.
W&B itself is out of scope.
"""
from __future__ import annotations

import gc
import math
import os
import time
from types import SimpleNamespace
from typing import Any, Dict, List, Optional

import torch
from torch import nn

from ..eval.eval import evaluate_clip
from ..model.build import instantiate
from ..model.losses import CORE_LOSS_KEY, BCECategoryLoss, MultiStepMultiMasksAndIous
from .ddp import ArenaGradReducer
from .optim import ArenaAdamW, ArenaOptimizer, cosine_with_warmup

try:  # the reference's base classes when Lightning is installed (it is not in this image)
    import lightning.pytorch as _pl
    _ModuleBase, _DataBase, HAVE_LIGHTNING = _pl.LightningModule, _pl.LightningDataModule, True
except Exception:  # pragma: no cover - depends on the environment
    _ModuleBase, _DataBase, HAVE_LIGHTNING = nn.Module, object, False


def _ns(x):
    if isinstance(x, dict):
        return SimpleNamespace(**{k: _ns(v) for k, v in x.items()})
    return x


def _get(ns, k, default=None):
    if ns is None:
        return default
    if isinstance(ns, dict):
        return ns.get(k, default)
    return getattr(ns, k, default)


def _todict(x):
    if isinstance(x, SimpleNamespace):
        return {k: _todict(v) for k, v in vars(x).items()}
    if hasattr(x, "items") and not isinstance(x, dict):  # OmegaConf DictConfig
        return {k: _todict(v) for k, v in x.items()}
    return x


def precision_dtype(precision) -> str:
    """Lightning `precision` -> compute dtype of the kernels.  "16"/"16-mixed" (fp16 AMP in the
    reference configs, best.yaml:103) and "bf16*" run bf16 (same width; fp16 is not a CDNA4
    training format here), "32*"/"64*" run the fp32 mode, "fp8" / "transformer-engine" the MX-fp8
    mode."""
    p = str(precision if precision is not None else "bf16").lower()
    if p.startswith("fp8") or p.startswith("mxfp8") or p == "transformer-engine":
        return "fp8"  # MX-fp8 projections / FFN (BASELINE config 5, kernels/fp8.py)
    return "fp32" if p.startswith("32") or p.startswith("64") else "bf16"


class SAM2LightningModule(_ModuleBase):
    def __init__(self, model: Any, loss: Any, optimizer: Any, scheduler: Any, visualization: Any = None, *,
                 gradient_clip_val: Optional[float] = None, accumulate_grad_batches: Optional[int] = None):
        """The reference's five sections (trainer.py:38-99).  Under a Lightning Trainer the module uses
        Lightning's automatic optimization exactly as the reference does: the Trainer's
        gradient_clip_val and accumulate_grad_batches (best.yaml:105-106) apply as configured
        (configure_optimizers returns a torch.optim.Optimizer over the gradient arena,
        configure_gradient_clipping routes the clip into its fused kernel).  The two keyword-only
        extras are the same settings for this build's StepRunner when it is driven without a
        Trainer; this build's Trainer sets them from its own arguments."""
        super().__init__()
        cfg = SimpleNamespace(model=model, loss=_ns(_todict(loss)), optimizer=_ns(_todict(optimizer)),
                              scheduler=_ns(_todict(scheduler)), visualization=_ns(_todict(visualization or {})))
        if HAVE_LIGHTNING:  # pragma: no cover
            self.save_hyperparameters(ignore=["model"] if isinstance(model, nn.Module) else None)
        else:
            self.hparams = cfg
        self.cfg = cfg
        self.model = None
        L = cfg.loss
        lt = _get(L, "type", None)
        if lt is not None and str(lt).lower() in {"bce", "bce_only", "ce_only"}:
            self.criterion = BCECategoryLoss(pos_weight=_get(L, "bce_pos_weight"),
                                             reduction=_get(L, "bce_reduction", "mean"),
                                             logit_temperature=_get(L, "bce_logit_temperature", 1.0))
        else:
            self.criterion = MultiStepMultiMasksAndIous(
                weight_dict=_todict(_get(L, "weight_dict")), supervise_all_iou=_get(L, "supervise_all_iou", False),
                iou_use_l1_loss=_get(L, "iou_use_l1_loss", False), pred_obj_scores=_get(L, "pred_obj_scores", False),
                focal_gamma_obj_score=_get(L, "focal_gamma_obj_score", 0.0),
                focal_alpha_obj_score=_get(L, "focal_alpha_obj_score", -1.0),
                logit_temperature=_get(L, "multistep_logit_temperature", 1.0))
        self.loss_gt_stride = max(int(_get(L, "gt_stride", 1)), 1)
        self.logged: Dict[str, Any] = {}
        self.optimizer = None
        self.lr_at = None
        # clip / accumulation of the StepRunner (this build's Trainer overwrites them with its own
        # arguments; under Lightning the Trainer's own settings apply)
        self.gradient_clip_val = gradient_clip_val
        self.accumulate_grad_batches = accumulate_grad_batches
        self.compute_dtype = None  # set by the Trainer from `precision` (Lightning: setup reads it)
        self.last_visualization: Optional[Dict[str, Any]] = None  # what _log_gif wrote last

    # ------------------------------------------------------------ setup
    def setup(self, stage: str = "fit", device=None):
        """trainer.py:101-115: instantiate the model section, load it on the device (the current
        CUDA device -- the rank's own under DDP -- when none is given), train mode"""
        if stage == "fit":
            tr = self._attached_trainer()
            if self.compute_dtype is None and tr is not None and getattr(tr, "precision", None) is not None:
                self.compute_dtype = precision_dtype(tr.precision)  # Lightning's "16-mixed" etc.
            if self.model is None:
                m = self.cfg.model
                if isinstance(m, nn.Module):
                    self.model = m
                else:
                    kw = {"compute_dtype": self.compute_dtype} if self.compute_dtype else {}
                    self.model = instantiate(_todict(m), **kw)
            if device is None:
                device = torch.device("cuda", torch.cuda.current_device())
            self.model.load(device)
            self.model.train()

    def configure_optimizers(self, total_steps: Optional[int] = None) -> Optional[Dict[str, Any]]:
        """trainer.py:117-177: AdamW(lr, weight_decay, betas) -- eps 1e-8 / amsgrad False whatever the
        YAML says -- with get_cosine_schedule_with_warmup(total * warmup_factor, total), stepped per
        optimizer step.  The clip is the Trainer's gradient_clip_val (Lightning's clip_grad_norm_).
        Called by Lightning (no argument, a trainer attached): ArenaOptimizer, a torch.optim.Optimizer
        over the gradient arena, with a LambdaLR of that schedule over the trainer's
        estimated_stepping_batches (optimizer steps: Lightning counts them with its own
        accumulate_grad_batches and max_steps).  Called by StepRunner (total_steps given): the arena
        AdamW and the schedule as a step -> lr function."""
        o = self.cfg.optimizer
        if str(_get(o, "type", "adamw")).lower() != "adamw":
            raise NotImplementedError("only AdamW (the reference configs' optimizer) is built")
        tr = self._attached_trainer()
        if total_steps is None and tr is not None:
            return self._lightning_optimizers(tr)
        total_steps = 1 if total_steps is None else total_steps
        opt = ArenaAdamW(self.model.arena, lr=_get(o, "lr", 1e-4), weight_decay=_get(o, "weight_decay", 0.01),
                         betas=tuple(_get(o, "betas", (0.9, 0.999))), eps=1e-8,
                         max_grad_norm=self.gradient_clip_val)
        self.optimizer = opt
        sched = None
        if _get(self.cfg.scheduler, "enabled", True):
            total = max(1, int(total_steps))
            warm = total * float(_get(o, "warmup_factor", 0.0))
            if warm >= total:
                warm = max(0, total - 1)
            self.lr_at = cosine_with_warmup(opt.lr, warm, total, float(_get(self.cfg.scheduler, "num_cycles", 0.5)))
            sched = {"scheduler": self.lr_at, "interval": "step", "frequency": 1}
        return {"optimizer": opt, "lr_scheduler": sched} if sched else {"optimizer": opt}

    def _lightning_optimizers(self, tr) -> Dict[str, Any]:
        o = self.cfg.optimizer
        params = [p for p in self.model.parameters() if getattr(p, "_s2h_grad", None) is not None]
        lr = float(_get(o, "lr", 1e-4))
        acc = int(getattr(tr, "accumulate_grad_batches", 1) or 1)
        if self.accumulate_grad_batches not in (None, 1, acc):
            self._warn_once("acc", "SAM2LightningModule(accumulate_grad_batches=%s) is ignored under a Lightning "
                            "Trainer, whose accumulate_grad_batches=%s applies" % (self.accumulate_grad_batches, acc))
        opt = ArenaOptimizer(self.model.arena, params, lr=lr, weight_decay=_get(o, "weight_decay", 0.01),
                             betas=tuple(_get(o, "betas", (0.9, 0.999))), eps=1e-8,
                             max_grad_norm=getattr(tr, "gradient_clip_val", None) or 0.0)
        self.optimizer = opt
        if not _get(self.cfg.scheduler, "enabled", True):
            return {"optimizer": opt}
        total = max(1, int(getattr(tr, "estimated_stepping_batches", 1)))
        warm = total * float(_get(o, "warmup_factor", 0.0))
        if warm >= total:
            warm = max(0, total - 1)
        self.lr_at = cosine_with_warmup(lr, warm, total, float(_get(self.cfg.scheduler, "num_cycles", 0.5)))
        sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda step: self.lr_at(step) / lr)
        return {"optimizer": opt, "lr_scheduler": {"scheduler": sched, "interval": "step", "frequency": 1}}

    def configure_gradient_clipping(self, optimizer, gradient_clip_val=None, gradient_clip_algorithm=None):
        """Lightning hook (automatic optimization, before each optimizer step): the Trainer's
        gradient_clip_val becomes the fused AdamW kernel's clip (clip_grad_norm_, norm type 2, on the
        device, no host sync) instead of torch's clip over every `p.grad`.  With no clip on the Trainer
        the module's own gradient_clip_val keyword (the StepRunner setting) applies, with a warning."""
        if gradient_clip_algorithm not in (None, "norm"):
            raise NotImplementedError("gradient_clip_algorithm='value' is not built (the reference clips by norm)")
        if gradient_clip_val is None and self.gradient_clip_val:
            self._warn_once("clip", "SAM2LightningModule(gradient_clip_val=%s) applies: the Lightning Trainer sets no "
                            "gradient_clip_val (set it on the Trainer, as best.yaml:105 does)" % self.gradient_clip_val)
            gradient_clip_val = self.gradient_clip_val
        opt = getattr(optimizer, "_optimizer", optimizer)  # LightningOptimizer wraps the optimizer
        opt.max_grad_norm = float(gradient_clip_val or 0.0)

    def _warn_once(self, key, msg):
        seen = self.__dict__.setdefault("_warned", set())
        if key not in seen:
            seen.add(key)
            import warnings
            warnings.warn(msg, UserWarning, stacklevel=3)

    def backward(self, loss, *args, **kwargs):
        """Lightning hook (automatic optimization): a no-op after the graph-replayed micro-step (its
        backward already filled the gradient arena inside training_step); otherwise loss.backward()
        with the gradient arena's deferred fixed-order sums flushed at its end
        (kernels.ops.deferred_grad_sums) and, on the last micro-batch of an accumulation window under
        DDP, the arena all-reduce -- before the precision plugin's GradScaler unscales and checks the
        gradients for inf / NaN, so every rank sees the same reduced gradients and takes the same
        skip-or-step decision (what DistributedDataParallel's in-backward reduce guarantees)"""
        if self.__dict__.pop("_pl_grads_ready", False):
            return
        from ..kernels.ops import deferred_grad_sums
        with deferred_grad_sums(self.model.arena.grad_region()):
            loss.backward(*args, **kwargs)
        if self.__dict__.pop("_pl_window_end", False):
            opt = self.optimizer
            if opt is not None and hasattr(opt, "reduce_now"):
                opt.reduce_now()

    # --------------------------------------------------------- forward
    def forward(self, batch):
        """trainer.py:182-188"""
        return self.model(batch)

    def _apply_gt_stride(self, outs_per_frame, target_masks):
        """trainer.py:190-203"""
        if self.loss_gt_stride <= 1:
            return outs_per_frame, target_masks
        idxs = list(range(0, len(outs_per_frame), self.loss_gt_stride))
        return [outs_per_frame[i] for i in idxs], target_masks[idxs]

    def log(self, name, value, **kw):
        self.logged[name] = value.detach() if torch.is_tensor(value) else value
        # not while a StepRunner records / captures the step: Lightning's metric updates would be
        # captured into the graph; the graph-replayed path logs the step's values after each replay
        if HAVE_LIGHTNING and self._attached_trainer() is not None and not self.__dict__.get("_in_runner"):
            super().log(name, value, batch_size=1, **kw)  # pragma: no cover

    # Under a Lightning Trainer (automatic optimization) training_step runs the whole micro-step --
    # forward, loss and the backward into the gradient arena -- as a replay of the captured HIP graph
    # (StepRunner's, the bench path) and returns the loss; the backward hook is then a no-op.  False:
    # the eager module (Lightning's own training_step -> backward order, no graph).
    lightning_graph = True

    def _pl_runner(self, tr, k):
        run = self.__dict__.get("_pl_run")
        if run is None or run.accumulate != k:
            import torch.distributed as dist
            world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
            run = StepRunner(self, graph=True, distributed=world > 1, accumulate_grad_batches=k, optimizer=False)
            self._pl_run = run
        return run

    @staticmethod
    def _pl_is_window_end(tr, batch_idx, k):
        """Lightning steps the optimizer after this micro-batch (fit_loop._should_accumulate() is
        False): the k-th batch of a window or the epoch's last batch"""
        loop = getattr(tr, "fit_loop", None)
        fn = getattr(loop, "_should_accumulate", None)
        if fn is not None:
            return not fn()
        n = getattr(tr, "num_training_batches", None)
        return (batch_idx + 1) % k == 0 or (isinstance(n, int) and batch_idx + 1 >= n)

    def _pl_graphed_step(self, batch, batch_idx, tr):
        """one Lightning micro-batch through the StepRunner: the arena is zeroed when the window starts
        (Lightning's zero_grad, which follows training_step in its closure, is then skipped for this
        micro-batch), the backward is seeded with the precision plugin's GradScaler scale (so
        unscale_ / the inf check see what loss.backward() of the scaled loss would have produced), and on
        the window's last micro-batch under DDP the arena ranges are all-reduced beside the staged
        backbone backward, as StepRunner overlaps them.  Lightning's 1/accumulate_grad_batches loss
        normalisation is folded into the optimizer step's gradient scale (ArenaOptimizer.window_scale),
        as StepRunner folds it: the arena holds the window's summed gradients, bit-identical to the
        StepRunner's."""
        k = max(1, int(getattr(tr, "accumulate_grad_batches", 1) or 1))
        run = self._pl_runner(tr, k)
        end = self._pl_is_window_end(tr, batch_idx, k)
        scaler = getattr(getattr(tr, "precision_plugin", None), "scaler", None)
        loss = run.lightning_micro_step(batch, window_start=batch_idx % k == 0, reduce=end, scaler=scaler)
        opt = self.optimizer
        if opt is not None:
            opt.hold_grads = batch_idx % k == 0  # the zero_grad Lightning issues after this training_step
            if end:
                opt.window_scale = 1.0 / k
                opt.reduced = run.reducer is not None
        self._pl_grads_ready = True
        if HAVE_LIGHTNING:  # pragma: no cover
            for name, v in self.logged.items():
                super().log(name, v, batch_size=1)
        return loss

    def training_step(self, batch, batch_idx: int = 0) -> torch.Tensor:
        """trainer.py:256-289: forward, the loss on the gt_stride frames, the logged terms; returns
        the loss (Lightning / StepRunner run the backward into the gradient arena).  Under a Lightning
        Trainer with lightning_graph (default) the micro-step is the StepRunner's graph replay
        (_pl_graphed_step)."""
        tr = self._attached_trainer()
        if tr is not None and not self.__dict__.get("_in_runner"):
            if self.lightning_graph:
                return self._pl_graphed_step(batch, batch_idx, tr)
            k = max(1, int(getattr(tr, "accumulate_grad_batches", 1) or 1))
            self._pl_window_end = self._pl_is_window_end(tr, batch_idx, k)
        outs_per_frame, obj_to_cat = self.forward(batch)
        self.last_outputs = outs_per_frame
        outs, targets = self._apply_gt_stride(outs_per_frame, batch.masks)
        losses = self.criterion(outs, targets)
        total = losses[CORE_LOSS_KEY]
        self.log("train/total_loss", total)
        for k, v in losses.items():
            if k in (CORE_LOSS_KEY, "logits"):
                continue
            self.log(f"train/{k}", v)
        if self.optimizer is not None:
            self.log("train/learning_rate", self.optimizer.param_groups[0]["lr"])
        # (a graph-replaying StepRunner runs the hook itself after the replay: this body is then a warm-up or a
        # capture, and the captured outputs' point inputs are those of the first clip)
        deferred = self.__dict__.get("_in_runner") and self.__dict__.get("_viz_deferred")
        if not deferred and self._should_log_gif("train", batch_idx):
            self._log_gif("train", batch.img_batch.squeeze(1), batch.masks, outs_per_frame, obj_to_cat, "train")
        return total

    # --------------------------------------------------- visualisation
    def _fit_trainer(self):
        """the trainer of the running fit: Lightning's, or this build's (Trainer.fit sets `trainer_`)"""
        return self._attached_trainer() or self.__dict__.get("trainer_")

    def _batches_ready(self, tr) -> int:
        """training batches started in this fit, the current one included (1 on the first): Lightning's
        fit_loop.epoch_loop.batch_progress.total.ready; this build's Trainer counts epoch * batches per epoch +
        the batch's index + 1 (both restored by a resume; the same number as the micro-step counter less the
        padding of partial accumulation windows at epoch ends); a bare StepRunner its micro-steps"""
        prog = getattr(getattr(getattr(tr, "fit_loop", None), "epoch_loop", None), "batch_progress", None)
        if prog is not None:
            return int(prog.total.ready)
        if getattr(tr, "batches_ready", None) is not None:
            return int(tr.batches_ready)
        return int(self.__dict__.get("_viz_ready", 0))

    def _should_log_gif(self, split: str, batch_idx: int) -> bool:
        """trainer.py:206-223: never unless visualization.enabled and on global rank 0; train: every
        train_every_n_steps-th started batch (0 = never); val: the first batch of every
        val_first_batch_every_n_epochs-th epoch (0 = every epoch)"""
        viz = self.cfg.visualization
        if not _get(viz, "enabled", False):
            return False
        tr = self._fit_trainer()
        zero = getattr(tr, "is_global_zero", None)
        if zero is None:
            import torch.distributed as dist
            zero = not (dist.is_available() and dist.is_initialized()) or dist.get_rank() == 0
        if not zero:
            return False
        if split == "train":
            steps = int(_get(viz, "train_every_n_steps", 0) or 0)
            return steps > 0 and self._batches_ready(tr) % steps == 0
        if split == "val":
            epochs = int(_get(viz, "val_first_batch_every_n_epochs", 0) or 0)
            if epochs == 0:
                return batch_idx == 0
            return batch_idx == 0 and int(getattr(tr, "current_epoch", 0)) % epochs == 0
        return False

    def _log_gif(self, stage: str, frames, gt_masks, outs_per_frame, obj_to_cat, split: str):
        """trainer.py:225-252 with a file in place of wandb.Video: nothing unless visualization.save_dir is set;
        else the composites (device kernels, one copy back through the pinned staging buffer) go to
        <save_dir>/{split}_e{epoch:04d}_s{global_step:07d}.gif at 4 fps with the reference's caption as the GIF
        comment.  Never inside a stream capture."""
        viz = self.cfg.visualization
        save_dir = _get(viz, "save_dir")
        if not save_dir or torch.cuda.is_current_stream_capturing():
            return None
        from ..utils import create_visualization_gif, save_visualization
        gif = create_visualization_gif(frames=frames, gt_masks=gt_masks, outs_per_frame=outs_per_frame,
                                       obj_to_cat=obj_to_cat, max_length=int(_get(viz, "max_length", 4)),
                                       stride=int(_get(viz, "stride", 1)), to_host=True)
        tr = self._fit_trainer()
        # (a StepRunner driven without a Trainer: epoch 0 and the runner's own optimizer-step count)
        epoch = int(getattr(tr, "current_epoch", 0))
        step = int(getattr(tr, "global_step", self.__dict__.get("_viz_global_step", 0)))
        caption = f"{_get(viz, 'caption', '')} | {split} e{epoch} s{step}"
        path = os.path.join(str(save_dir), f"{split}_e{epoch:04d}_s{step:07d}.gif")
        files = save_visualization(gif, path, fps=4, caption=caption, format=str(_get(viz, "format", "gif")))
        self.last_visualization = {"stage": stage, "path": path, "files": files, "caption": caption,
                                   "array": gif.copy()}  # (gif is a view of the reused staging buffer)
        return path

    def _attached_trainer(self):
        """the Lightning trainer driving this module (LightningModule._trainer), if any; this
        build's own Trainer drives StepRunner directly and does not attach itself"""
        return getattr(self, "_trainer", None)

    @torch.no_grad()
    def validation_step(self, batch, batch_idx: int = 0) -> torch.Tensor:
        """trainer.py:291-322 (loss, no gradient tape) in eval mode (dropout off, as Lightning's
        model.eval() before validation) plus the reference's offline evaluation metrics computed in
        the loop on every frame (eval/eval.py: IoU / Dice / MAE of the category-merged binarised
        masks, averaged as get_video_scores does): val/iou, val/dice, val/mae."""
        was = self.model.training
        self.model.eval()
        try:
            outs_per_frame, obj_to_cat = self.forward(batch)
            outs, targets = self._apply_gt_stride(outs_per_frame, batch.masks)
            losses = self.criterion(outs, targets)
        finally:
            self.model.train(was)
        self.log("val/total_loss", losses[CORE_LOSS_KEY])
        for k, v in losses.items():
            if k not in (CORE_LOSS_KEY, "logits"):
                self.log(f"val/{k}", v)
        scores = evaluate_clip(outs_per_frame, batch.masks)
        self.last_eval = scores
        for k, v in scores["avg_scores"].items():
            self.log(f"val/{k}", v)
        if self._should_log_gif("val", batch_idx):
            self._log_gif("val", batch.img_batch.squeeze(1), batch.masks, outs_per_frame, obj_to_cat, "val")
        return losses[CORE_LOSS_KEY]


class StepRunner:
    """One micro-step of the fit loop: (zero the arena when a window starts) -> training_step ->
    backward into the gradient arena, and at every `accumulate_grad_batches`-th micro-step: RCCL
    all-reduce (N > 1) -> clip + AdamW (+ schedule).  Everything stays on the device.

    Gradient accumulation follows Lightning: micro-step gradients are summed, the loss scale
    1/accumulate (and the 1/world average of DDP) is folded into the optimizer's grad_scale, the
    clip sees the scaled gradient, the schedule counts optimizer steps, and non-boundary
    micro-steps issue no all-reduce (DDP no_sync).

    graph=True captures forward + loss + backward of a micro-step ONCE per input signature
    (frame count, image size, category/object layout) into a HIP graph and replays it: the ~5k
    kernel launches of a B+ 512^2 8-frame step cost one graph launch instead of ~5k Python/ctypes
    launches.  Per step only the host prompt stage (connected components + clicks,
    sam2model.py:181-236), the copies of the new clip into the graph's static input buffers, the
    dropout RNG offset and the boundary work (all-reduce, optimizer, zeroing) run eagerly.
    Dropout masks still change every step: kernels fold the device-resident RNG offset into
    their seeds (s2h_rng_bind)."""

    def __init__(self, module: SAM2LightningModule, total_steps: int = 1, distributed: bool = False,
                 graph: bool = False, accumulate_grad_batches: int = 1, gradient_clip_val=None,
                 split_backward: Optional[bool] = None, optimizer: bool = True):
        """optimizer=False: the Lightning path (SAM2LightningModule._pl_graphed_step) -- the runner
        only runs micro-steps (lightning_micro_step); Lightning's optimizer loop steps the module's
        ArenaOptimizer"""
        self.module = module
        if gradient_clip_val is not None:
            module.gradient_clip_val = gradient_clip_val
        if optimizer:
            module.configure_optimizers(total_steps)
        arena = module.model.arena
        self.reducer = ArenaGradReducer(arena.grad_region(), split=arena.grad_split) if distributed else None
        # overlap: a two-phase backward -- (1) loss -> backbone outputs (the frame-batched
        # tracking backward completes every gradient except the backbone's), (2) the backbone's
        # backward in segments (SAM2Model.backbone_backward_segments: conv_s0/s1 + neck, then the
        # Hiera stages last to first) -- with the all-reduce of every completed arena range
        # (arena.grad_cuts) issued as soon as its segment ends, beside the following segments
        self.cuts = list(getattr(arena, "grad_cuts", [arena.grad_split, arena.n_grad]))
        split_ok = getattr(module.model, "frame_batched", False) and arena.grad_split < arena.n_grad
        self.overlap = bool(split_ok and (distributed if split_backward is None else split_backward))
        self.accumulate = max(1, int(accumulate_grad_batches or 1))
        self.global_step = 0  # optimizer steps
        self.micro_step = 0
        # a learning rate that replaces the schedule's until it is set back to None (the SWA phase:
        # Trainer.set_epoch_lr, training/callbacks.py StochasticWeightAveraging)
        self.lr_override: Optional[float] = None
        self.graph = graph
        self._graphs: Dict[Any, Dict[str, Any]] = {}
        self.before_capture = None  # optional callable, run right before a graph is captured
        from ..kernels import functional as FN
        from ..kernels.ops import deferred_grad_sums, rng_offset
        self._fn = FN
        self._sums = lambda: deferred_grad_sums(module.model.arena.grad_region())
        self.rng = rng_offset(module.model.arena.device)
        # every step (eager, warm-up, capture) draws the same per-launch host seeds; the step-to-step
        # variation of the dropout masks comes from the device RNG offset alone, so an eager step
        # and a replay of the captured one use identical masks
        self.seed_base = FN._SEED[0]
        self._pending = None
        self._segs = None
        # the backward's seed dL/dL: 1 (StepRunner), or the GradScaler scale of the Lightning path;
        # a device tensor read by the loss kernels' backward, so a captured graph picks up new values
        self.grad_seed = torch.ones((), device=arena.device, dtype=torch.float32)
        # the visualisation hook of a graph-replayed step runs after the replay (_visualize), not in training_step
        module._viz_deferred = bool(graph)
        self._last_ent = None
        module.model.arena.zero_grad()

    def _device_step(self, batch):
        """forward + loss + backward (phase 1 only when overlapping; _phase2 finishes it)"""
        self._fn.set_seed(self.seed_base)
        m = self.module
        m._in_runner = True
        try:
            loss = m.training_step(batch, self.micro_step)
        finally:
            m._in_runner = False
        seed = self.grad_seed.view(loss.shape)
        bb = getattr(m.model, "last_backbone_outputs", None) if self.overlap else None
        with self._sums():  # each backward phase flushes its deferred gradient sums at its end
            if bb:
                grads = torch.autograd.grad(loss, bb, grad_outputs=seed, allow_unused=True)
                self._pending = [(t, g) for t, g in zip(bb, grads) if g is not None]
            else:
                self._pending = None
                loss.backward(seed)
        return loss

    def _segments(self):
        """the pending phase-2 backward as [(closure, arena rank)] (consumes the pending state)"""
        pend = self._pending
        self._pending = None
        if not pend:
            return []
        segs = getattr(self.module.model, "backbone_backward_segments", None)
        if segs is None:
            segs = [(lambda: torch.autograd.backward([t for t, _ in pend], [g for _, g in pend]), 0)]
        else:
            segs = segs(pend)

        def phase(run):
            def f():
                with self._sums():
                    run()
            return f
        return [(phase(run), rank) for run, rank in segs]

    def _phase2(self):
        for run, _ in self._segments():
            run()

    def _graphed_step(self, batch):
        model = self.module.model
        dev = model.arena.device
        plan = model.host_prompt_plan(batch)
        key = (tuple(batch.img_batch.shape), tuple(batch.masks.shape), tuple(plan["obj_to_cat"]),
               plan["num_categories"], tuple(t.shape for t in plan["host"]))
        ent = self._graphs.get(key)
        if ent is None:
            static = _static_batch(batch, dev)
            plan = dict(plan)
            plan["dev"] = model.upload_prompt_plan(plan, dev)
            static.prompt_plan = plan
            # the eager warm-up accumulates into the gradient arena: keep what earlier micro-steps
            # of this accumulation window left there
            saved = model.arena.grad_region().clone() if self.micro_step % self.accumulate else None
            cur = torch.cuda.current_stream(dev)
            side = torch.cuda.Stream(dev)
            side.wait_stream(cur)
            with torch.cuda.stream(side):  # eager warm-up: fills every device-side table cache
                self._device_step(static)
                self._phase2()
            cur.wait_stream(side)
            if saved is not None:
                model.arena.grad_region().copy_(saved)
            else:
                model.arena.zero_grad()
            if self.before_capture is not None:
                self.before_capture()
            # A dead Python cycle can hold an earlier fit's captured graphs and their private pool (trainer
            # <-> module <-> runner: Trainer.fit sets module.trainer_).  Collected while this capture is
            # open, its graphs and pool would be destroyed inside the capture -- the process has aborted in
            # exactly that state ("Garbage-collecting" under the capture below, no message).  torch.cuda.graph
            # no longer collects on entry (torch >= 2.9: only with force_cudagraph_gc), so collect here.
            gc.collect()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                loss = self._device_step(static)
            segs = []
            for run, rank in self._segments():  # the backbone's backward: one graph per segment
                gk = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gk, pool=g.pool()):
                    run()
                segs.append((gk.replay, rank, gk))
            ent = self._graphs[key] = {"graph": g, "segs": segs, "batch": static, "loss": loss,
                                       "logged": dict(self.module.logged), "outputs": self.module.last_outputs}
        else:
            st = ent["batch"]
            st.img_batch.copy_(batch.img_batch, non_blocking=True)
            st.masks.copy_(batch.masks, non_blocking=True)
            st.obj_to_frame_idx.copy_(batch.obj_to_frame_idx, non_blocking=True)
            model.upload_prompt_plan(plan, dev, out=st.prompt_plan["dev"])
            st.prompt_plan.update({k: plan[k] for k in ("points", "labels")})
        ent["graph"].replay()
        self._last_ent = ent
        self._segs = [(rep, rank) for rep, rank, _ in ent["segs"]]
        self.module.logged = dict(ent["logged"])
        self.module.last_outputs = ent["outputs"]
        return ent["loss"]

    def begin_micro_step(self):
        """zero the gradient arena when an accumulation window starts (Lightning's zero_grad) and
        draw fresh dropout masks (the device RNG offset); shared by __call__ and the Lightning path"""
        if self.micro_step % self.accumulate == 0:
            self.module.model.arena.zero_grad()
        self.rng.fill_(self.micro_step + 1)
        self._fn.set_seed(self.seed_base)

    def flush(self) -> bool:
        """close a partial accumulation window (Lightning steps the optimizer on an epoch's last
        batch even when fewer than accumulate_grad_batches micro-steps were taken)"""
        if self.micro_step % self.accumulate == 0:
            return False
        self.micro_step += self.accumulate - self.micro_step % self.accumulate - 1
        return self.after_backward()

    def after_backward(self, reduced: bool = False) -> bool:
        """Counts the micro-step; at an accumulation boundary runs all-reduce (unless `reduced`:
        __call__ already overlapped it with the backward) + clip + AdamW (the arena is zeroed when
        the next window starts).  Returns True when an optimizer step was taken."""
        m = self.module
        self.micro_step += 1
        if self.micro_step % self.accumulate:
            return False
        scale = 1.0 / self.accumulate
        if self.reducer is not None:
            if not reduced:
                self.reducer.reduce()
            scale *= self.reducer.grad_scale
        lr = self.next_lr()
        m.optimizer.step(lr=lr, grad_scale=scale)
        m.log("train/learning_rate", m.optimizer.param_groups[0]["lr"])
        self.global_step += 1
        return True

    def next_lr(self) -> Optional[float]:
        """the rate the next optimizer step is given: the override, else the schedule's (None: the optimizer
        keeps the rate it holds)"""
        if self.lr_override is not None:
            return self.lr_override
        m = self.module
        return m.lr_at(self.global_step) if m.lr_at is not None else None

    def discard_window(self):
        """drop an open, partial accumulation window without stepping (the fit loop leaves on should_stop):
        the next micro-step starts a new window and zeroes the arena"""
        self.micro_step -= self.micro_step % self.accumulate

    def __call__(self, batch):
        self.begin_micro_step()
        loss = self._run(batch, (self.micro_step + 1) % self.accumulate == 0)
        self.after_backward(reduced=self.overlap and self.reducer is not None
                            and (self.micro_step + 1) % self.accumulate == 0)
        return loss

    def lightning_micro_step(self, batch, window_start: bool, reduce: bool, scaler=None):
        """The Lightning path's micro-step (no optimizer step: Lightning's optimizer loop takes it):
        zero the arena when the accumulation window starts, draw fresh dropout masks, seed the backward
        with the GradScaler's current scale (device tensor, no host sync; its init_scale before the
        first scale() call; 1 without a scaler), forward + loss + backward (graph replay), and when
        `reduce` (the window's last micro-batch) under DDP the arena all-reduce of every range beside
        the staged backward, finished before this returns -- so Lightning's unscale_ / inf check /
        clip see the reduced gradients on every rank."""
        if window_start:
            self.module.model.arena.zero_grad()
        self.rng.fill_(self.micro_step + 1)
        self._fn.set_seed(self.seed_base)
        if scaler is not None and getattr(scaler, "is_enabled", lambda: True)():
            s = getattr(scaler, "_scale", None)
            if s is None:
                self.grad_seed.fill_(float(getattr(scaler, "_init_scale", 1.0)))
            else:
                self.grad_seed.copy_(s.reshape(()))
        else:
            self.grad_seed.fill_(1.0)
        loss = self._run(batch, reduce)
        if reduce and self.reducer is not None and not self.overlap:
            self.reducer.reduce()
        self.micro_step += 1
        return loss

    def _run(self, batch, boundary):
        """forward + loss + backward of one micro-step (graph replay or eager); at an accumulation
        boundary under DDP with the staged backward, each completed arena range is all-reduced beside
        the following segments (the works are waited for before this returns)"""
        self._segs = None
        # (the batch and optimizer-step counts of a runner driven without a Trainer, for the visualisation)
        self.module._viz_ready, self.module._viz_global_step = self.micro_step + 1, self.global_step
        loss = self._graphed_step(batch) if self.graph else self._device_step(batch)
        if self._segs is None:
            self._segs = self._segments()
        reduce = self.overlap and self.reducer is not None and boundary
        works = []
        if reduce:
            # the tracking gradients are complete: reduce them beside the backbone's backward
            works += self.reducer.reduce_range(0, self.cuts[0])
        done = 0  # arena ranks reduced so far
        for run, rank in self._segs:
            run()
            if reduce:  # this segment's range is complete: reduce it beside the next segments
                works += self.reducer.reduce_range(self.cuts[done], self.cuts[rank + 1])
                done = rank + 1
        self._segs = None
        if reduce:
            works += self.reducer.reduce_range(self.cuts[done], self.reducer.grad.numel())
            for w in works:
                w.wait()
        if self.graph:
            self._visualize()
        return loss

    def _visualize(self):
        """the training visualisation of a graph-replayed micro-step, after its device work is issued and outside
        every capture: the static batch, the outputs the replay just rewrote and the prompt plan's host points
        (the captured outputs carry the first clip's)"""
        m, ent = self.module, self._last_ent
        if ent is None or not m._should_log_gif("train", self.micro_step):
            return
        st = ent["batch"]
        plan = st.prompt_plan
        outs = list(ent["outputs"])
        if plan.get("points") is not None:
            outs[0] = dict(outs[0], point_inputs={"point_coords": plan["points"], "point_labels": plan["labels"]})
        m._log_gif("train", st.img_batch.squeeze(1), st.masks, outs, plan["obj_to_cat"], "train")


def _static_batch(batch, device):
    """device-resident copy of a batch whose tensors serve as a captured graph's input buffers"""
    from ..data.data_utils import BatchedVideoDatapoint
    out = BatchedVideoDatapoint(img_batch=batch.img_batch.to(device, copy=True),
                                obj_to_frame_idx=batch.obj_to_frame_idx.to(device, copy=True),
                                masks=batch.masks.to(device, copy=True), metadata=batch.metadata,
                                dict_key=batch.dict_key, batch_size=list(batch.batch_size))
    out.host_masks0 = None
    return out


def _to_device(batch, device):
    """a loader's batch on the device: copied, or, for the raw clips of `preprocess_on_device`, built there by
    the preprocessing kernels (data/preprocess.py) -- an ordinary device batch either way"""
    from ..data.preprocess import to_device_batch
    return to_device_batch(batch, device, non_blocking=True)


# ------------------------------------------------------------------ data module
class SAM2LightningDataModule(_DataBase):
    """trainer.py:325-400: B == 1 clip DataLoaders collated by sam2_collate_fn.  The data section
    (configs/data/*.yaml: train_path, val_path, image_size, video_clip_length, stride,
    num_workers, batch_size, num_categories) is read as the reference reads it; when the COCO
    annotation files are not present the loaders yield deterministic synthetic clips of the same
    shape (data/synthetic.py): `synthetic_clips` per split, clip indices from
    `synthetic_{train,val}_offset` (default 0 / 100000), `synthetic_objects` objects."""

    def __init__(self, data: Any, train_shuffle: bool = True):
        if _DataBase is not object:  # pragma: no cover
            super().__init__()
        self.data = _ns(_todict(data))
        self.train_shuffle = train_shuffle
        self.hparams = SimpleNamespace(data=self.data, train_shuffle=train_shuffle)
        self.train_dataset = None
        self.val_dataset = None

    def _dataset(self, split):
        d = self.data
        path = _get(d, f"{split}_path")
        if path and os.path.exists(str(path)):
            from ..data.dataset import COCODataset
            return COCODataset(config=d, coco_json_path=path)
        from ..data.synthetic import SyntheticClipDataset
        n_cat = int(_get(d, "num_categories", 13))
        return SyntheticClipDataset(num_clips=int(_get(d, "synthetic_clips", 16 if split == "train" else 4)),
                                    num_frames=int(_get(d, "video_clip_length", 8)),
                                    image_size=int(_get(d, "image_size", 512)), n_cat=n_cat,
                                    n_obj=int(_get(d, "synthetic_objects", n_cat)),
                                    offset=int(_get(d, f"synthetic_{split}_offset", 0 if split == "train" else 100_000)))

    def setup(self, stage: str = "fit"):
        if stage == "fit":
            self.train_dataset = self._dataset("train")
            self.val_dataset = self._dataset("val")

    def _loader(self, ds, shuffle):
        """B == 1 clip loader; with more than one rank in the process group the clips are sharded
        by a DistributedSampler (what Lightning injects under strategy=ddp): every rank trains on
        its own clips, the Trainer calls sampler.set_epoch each epoch"""
        import torch.distributed as dist
        from torch.utils.data import DataLoader, DistributedSampler

        from ..data.synthetic import sam2_collate_fn
        if ds is None:
            raise RuntimeError("dataset not initialized: call setup('fit') first")
        collate = sam2_collate_fn
        if getattr(getattr(getattr(ds, "video_dataset", None), "image_dataset", None), "preprocess_on_device", False):
            # COCO clips with `preprocess_on_device`: uint8 frames + RLE runs, finished on the device
            from ..data.preprocess import sam2_raw_collate_fn as collate
        sampler = None
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            sampler = DistributedSampler(ds, num_replicas=dist.get_world_size(), rank=dist.get_rank(),
                                         shuffle=shuffle)
        return DataLoader(ds, batch_size=int(_get(self.data, "batch_size", 1)),
                          num_workers=int(_get(self.data, "num_workers", 0)),
                          shuffle=shuffle if sampler is None else False, sampler=sampler,
                          pin_memory=torch.cuda.is_available(), collate_fn=collate)

    def train_dataloader(self):
        return self._loader(self.train_dataset, self.train_shuffle)

    def val_dataloader(self):
        return self._loader(self.val_dataset, False)


# ---------------------------------------------------------------------- trainer
class Trainer:
    """The `lightning.pytorch.Trainer` surface the reference configs use (best.yaml:98-113), driving
    SAM2LightningModule through StepRunner.  `callbacks` are driven as the module docstring says;
    other unknown Lightning arguments (logger, enable_progress_bar, ...) are accepted and ignored.
    With more than one rank the validation values in `callback_metrics` are the mean over the ranks
    (one small all-reduce per validation), so every rank's callbacks see the same monitored value and
    take the same decision; only rank 0 writes or deletes files."""

    def __init__(self, accelerator="auto", devices=1, precision=None, max_epochs=None, max_steps=-1,
                 gradient_clip_val=None, accumulate_grad_batches=1, val_check_interval=1.0,
                 num_sanity_val_steps=0, limit_train_batches=None, limit_val_batches=None,
                 log_every_n_steps=50, strategy="auto", graph=True, default_root_dir=None, callbacks=None,
                 **unused):
        if str(accelerator).lower() == "cpu":
            # the reference's config 1 (overfit.yaml, trainer.accelerator=cpu): this build's step is
            # HIP kernels only -- refuse rather than run on the GPU behind the caller's back
            raise ValueError("accelerator='cpu' is not supported: the sam2_video step runs as HIP kernels on an "
                             "MI355X (use accelerator='gpu' / 'auto')")
        self.accelerator = accelerator
        self.precision = precision
        self.devices = devices
        self.strategy = strategy
        self.max_epochs = max_epochs if max_epochs is not None else (1 if max_steps and max_steps > 0 else 1000)
        self.max_steps = int(max_steps if max_steps is not None else -1)
        self.gradient_clip_val = gradient_clip_val
        self.accumulate_grad_batches = max(1, int(accumulate_grad_batches or 1))
        self.val_check_interval = val_check_interval
        self.num_sanity_val_steps = int(num_sanity_val_steps or 0)
        self.limit_train_batches = limit_train_batches
        self.limit_val_batches = limit_val_batches
        self.log_every_n_steps = max(1, int(log_every_n_steps or 1))
        self.graph = graph
        self.default_root_dir = default_root_dir
        self.history: List[Dict[str, float]] = []
        self.val_history: List[Dict[str, float]] = []
        self.global_step = 0
        self.current_epoch = 0
        if callbacks is None:
            callbacks = []
        elif not isinstance(callbacks, (list, tuple)):
            callbacks = [callbacks]
        self.callbacks = list(callbacks)
        self.callback_metrics: Dict[str, float] = {}
        self.should_stop = False
        self.module = None
        self.runner = None
        self.batches_ready = 0  # training batches started in this fit (the visualisation schedule's counter)

    # ---------------------------------------------------------------- callbacks
    def _first_callback(self, name):
        from . import callbacks as C
        return next((cb for cb in self.callbacks if isinstance(cb, getattr(C, name))), None)

    @property
    def checkpoint_callback(self):
        """the first ModelCheckpoint of `callbacks`, or None"""
        return self._first_callback("ModelCheckpoint")

    @property
    def early_stopping_callback(self):
        return self._first_callback("EarlyStopping")

    @property
    def is_global_zero(self) -> bool:
        import torch.distributed as dist
        return not (dist.is_available() and dist.is_initialized()) or dist.get_rank() == 0

    def _call_hook(self, hook):
        """checkpoint callbacks go last (Lightning's order too), so the file one of them writes holds the
        other callbacks' state after they saw the same event"""
        from .callbacks import ModelCheckpoint
        for cb in sorted(self.callbacks, key=lambda cb: isinstance(cb, ModelCheckpoint)):
            fn = getattr(cb, hook, None)
            if fn is not None:
                fn(self, self.module)

    def _train_metrics(self):
        """the latest logged train/ values into callback_metrics (reads device scalars: called where a
        callback may look and at epoch ends, not per step)"""
        self.callback_metrics.update({k: float(v) for k, v in self.module.logged.items() if k.startswith("train/")})

    def current_lr(self) -> float:
        """the learning rate the next optimizer step will use"""
        lr = self.runner.next_lr()
        return float(lr if lr is not None else self.module.optimizer.param_groups[0]["lr"])

    def set_epoch_lr(self, lr: Optional[float]):
        """fix the learning rate of the following optimizer steps (None: back to the per-step schedule)"""
        self.runner.lr_override = None if lr is None else float(lr)

    @staticmethod
    def _limit(n, lim):
        if lim is None:
            return n
        if isinstance(lim, float) and lim <= 1.0:
            return int(n * lim)
        return min(n, int(lim))

    def _validate(self, module, loader, device, n):
        vals = []
        for i, batch in enumerate(loader):
            if i >= n:
                break
            module.validation_step(_to_device(batch, device), i)
            vals.append({k: float(v) for k, v in module.logged.items() if k.startswith("val/")})
        if vals:
            row = {k: sum(v[k] for v in vals) / len(vals) for k in vals[0]}
            # what callbacks decide on is the mean over the ranks (without callbacks: this rank's values)
            self.callback_metrics.update(self._mean_over_ranks(row, device) if self.callbacks else row)
            row["step"] = self.global_step
            self.val_history.append(row)

    @staticmethod
    def _mean_over_ranks(row, device):
        """with more than one rank: the mean of every value over the ranks, in one all-reduce of len(row) doubles
        (the ranks log the same keys)"""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
            return row
        keys = sorted(row)
        t = torch.tensor([row[k] for k in keys], dtype=torch.float64, device=device)
        dist.all_reduce(t)
        t /= dist.get_world_size()
        return dict(zip(keys, t.tolist()))

    def fit(self, module: SAM2LightningModule, datamodule=None, train_dataloaders=None, val_dataloaders=None,
            ckpt_path=None):
        """`ckpt_path` (Lightning's argument): continue the run a checkpoint of save_checkpoint was taken from,
        bit for bit (DESIGN.md §9 lists what is restored and why); a checkpoint without this build's resume block
        -- a Lightning / reference file -- restores weights, optimizer state, global_step and epoch, and the data
        starts at the beginning of that epoch.  What does not fit raises ValueError before the arena is written."""
        from . import resume as R
        from .ddp import init_from_env
        rank, world, local = init_from_env("nccl")
        device = torch.device("cuda", local)
        if world == 1:
            torch.cuda.set_device(device)
        if module.compute_dtype is None and self.precision is not None:
            module.compute_dtype = precision_dtype(self.precision)
        if datamodule is not None:
            datamodule.setup("fit")
            train_dataloaders = datamodule.train_dataloader()
            val_dataloaders = datamodule.val_dataloader()
        module.trainer_ = self
        self.module = module
        self.should_stop = False
        module.setup("fit", device)
        n_train = self._limit(len(train_dataloaders), self.limit_train_batches)
        n_val = self._limit(len(val_dataloaders), self.limit_val_batches) if val_dataloaders is not None else 0
        # Lightning's estimated_stepping_batches: a partial last window is an optimizer step too
        per_epoch = max(1, math.ceil(n_train / self.accumulate_grad_batches))
        total = self.max_steps if self.max_steps > 0 else per_epoch * self.max_epochs
        run = StepRunner(module, total, distributed=world > 1, graph=self.graph,
                         accumulate_grad_batches=self.accumulate_grad_batches,
                         gradient_clip_val=self.gradient_clip_val)
        self.runner = run
        self._batches_done, self._epoch_finished, self._rng_epoch_start = 0, False, None
        # every check of the checkpoint, then weights / optimizer / counters / an open window's gradients: before
        # on_fit_start, before anything is captured
        plan = self._plan_resume(ckpt_path, module, run, rank, world) if ckpt_path is not None else None
        if plan is not None:
            self._apply_resume(plan, module, run)
        self._call_hook("on_fit_start")  # (StochasticWeightAveraging allocates arena.swa here)
        if plan is not None:
            self._restore_callbacks(plan, module)
        if plan is not None and plan["complete"]:
            self._restore_books(plan)
            import warnings
            warnings.warn(f"Trainer.fit(ckpt_path={str(ckpt_path)!r}): the checkpoint's run is complete (epoch "
                          f"{plan['epoch']}, global_step {self.global_step}; max_epochs {self.max_epochs}, max_steps "
                          f"{self.max_steps}): nothing is trained", UserWarning, stacklevel=2)
            return self.history
        if n_val and self.num_sanity_val_steps:  # (the sanity validation triggers no callback)
            self._validate(module, val_dataloaders, device, min(n_val, self.num_sanity_val_steps))
            self.val_history.clear()
            self.callback_metrics.clear()
        start_epoch, skip = 0, 0
        if plan is not None:
            # after the sanity validation: its rows and its draws from the host generators leave no trace
            self._restore_books(plan)
            start_epoch, skip = plan["start_epoch"], plan["skip"]
            if plan["rng"] is not None and not plan["mid_epoch"]:
                R.set_host_rng_state(plan["rng"]["now"])
        vci = self.val_check_interval
        val_every = (max(1, int(n_train * vci)) if isinstance(vci, float) and vci <= 1.0 else int(vci)) if n_val else 0
        t0 = time.time()
        done = False
        for epoch in range(start_epoch, self.max_epochs):
            self.current_epoch = epoch
            sampler = getattr(train_dataloaders, "sampler", None)
            if hasattr(sampler, "set_epoch"):
                sampler.set_epoch(epoch)
            self._epoch_finished = False
            if plan is not None and plan["mid_epoch"] and epoch == start_epoch:
                # the interrupted epoch (its on_train_epoch_start ran before the checkpoint was taken): the
                # loader's iterator is created under the generator state the epoch started with, the consumed
                # batches are skipped in the sampler, then the state of the moment of the checkpoint is put back
                first = skip
                if plan["rng"] is not None:
                    self._rng_epoch_start = plan["rng"]["epoch_start"]
                    torch.set_rng_state(self._rng_epoch_start)
                batches = R.resumed_iterator(train_dataloaders, skip)
                if plan["rng"] is not None:
                    R.set_host_rng_state(plan["rng"]["now"])
            else:
                first = 0
                self._batches_done = 0
                self._call_hook("on_train_epoch_start")
                self._rng_epoch_start = torch.get_rng_state()
                batches = iter(train_dataloaders)
            for i, batch in enumerate(batches, first):
                if i >= n_train:
                    break
                before = run.global_step
                self.batches_ready = epoch * n_train + i + 1
                run(_to_device(batch, device))
                self.global_step = run.global_step
                self._batches_done = i + 1
                if run.global_step != before and run.global_step % self.log_every_n_steps == 0:
                    row = {k: float(v) for k, v in module.logged.items() if k.startswith("train/")}
                    row["step"], row["epoch"], row["time_s"] = run.global_step, epoch, time.time() - t0
                    self.history.append(row)
                if val_every and (i + 1) % val_every == 0:
                    self._validate(module, val_dataloaders, device, n_val)
                    if self.callbacks:
                        self._train_metrics()
                    self._call_hook("on_validation_end")
                    if self.should_stop:  # (EarlyStopping) leave right after this validation
                        run.discard_window()  # an open, partial accumulation window is not stepped
                        done = True
                        break
                if self.max_steps > 0 and run.global_step >= self.max_steps:
                    done = True
                    break
            if not done and run.flush():  # the epoch's last, partial accumulation window
                self.global_step = run.global_step
            self._epoch_finished = not done
            self._train_metrics()
            self._call_hook("on_train_epoch_end")
            if done:
                break
        self._call_hook("on_train_end")
        return self.history

    # ------------------------------------------------------------------- checkpoints
    def _world(self):
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            return dist.get_rank(), dist.get_world_size()
        return 0, 1

    def _resume_block(self, module):
        """this build's own block of a checkpoint (None outside a fit): counters, the host generators of every
        rank, an open accumulation window's partial sums of every rank, the SWA average, metrics and histories.
        Arena-shaped tensors go per parameter name (ParamArena.split).  With more than one rank this gathers from
        every rank, so every rank calls it; rank 0 gets the block, the others None."""
        from . import resume as R
        run = self.runner
        if run is None or module is not self.module or getattr(getattr(module, "model", None), "arena", None) is None:
            return None
        arena = module.model.arena
        rank, world = self._world()
        mine = {"epoch_start": self._rng_epoch_start, "now": R.host_rng_state(), "grads": None}
        if run.micro_step % run.accumulate:  # an open window: this rank's partial sums (not reduced yet)
            mine["grads"] = arena.split(arena.grad.detach().cpu(), "grad")
        ranks = [mine]
        if world > 1:
            import torch.distributed as dist
            ranks = [None] * world
            dist.all_gather_object(ranks, mine)
        if rank != 0:
            return None
        return {"version": R.FORMAT_VERSION, "world_size": world, "accumulate": run.accumulate,
                "micro_step": run.micro_step, "runner_global_step": run.global_step,
                "batches_done": int(self._batches_done), "epoch_finished": bool(self._epoch_finished),
                "seed_base": int(run.seed_base), "lr_override": run.lr_override,
                "trainable": arena.trainable_names(), "ranks": ranks,
                "swa": None if arena.swa is None else arena.split(arena.swa.detach().cpu(), "all"),
                "callback_metrics": dict(self.callback_metrics), "history": [dict(r) for r in self.history],
                "val_history": [dict(r) for r in self.val_history]}

    def save_checkpoint(self, path, module: Optional[SAM2LightningModule] = None):
        """Lightning-layout checkpoint: state_dict with the `model.` prefix (the reference strips it
        when it reloads, train.py:146-157), optimizer_states (torch.optim.AdamW's layout), lr_schedulers,
        callbacks ({state_key: state}), global_step and epoch, plus -- during and after a fit -- the block
        `s2h_resume` that fit(ckpt_path=...) needs for an exact resume.  Tensors, numbers, strings, lists and
        dicts only: it loads with weights_only=True.  Written by global rank 0 only (Lightning's rank-zero
        checkpointing; the parameters are identical on every rank), through a temporary file so that a job
        killed while writing leaves the previous file whole; with more than one rank every rank calls it
        (rank 0 collects the other ranks' generator states and open-window gradients).
        `module` defaults to the one being fitted (Lightning's trainer.save_checkpoint(path))."""
        from . import resume as R
        module = self.module if module is None else module
        block = self._resume_block(module)
        if self._world()[0] != 0:
            return
        sd = {"model." + k: v.detach().cpu() for k, v in module.model.state_dict().items()}
        ck = {"state_dict": sd, "optimizer_states": [module.optimizer.state_dict()],
              "global_step": self.global_step, "epoch": self.current_epoch, "lr_schedulers": [], "callbacks": {}}
        if getattr(module, "lr_at", None) is not None:  # torch LambdaLR's state at this optimizer step
            opt = module.optimizer
            ck["lr_schedulers"] = [{"base_lrs": [opt.lr], "last_epoch": self.global_step,
                                    "_step_count": self.global_step + 1, "lr_lambdas": [None],
                                    "_last_lr": [opt.param_groups[0]["lr"]]}]
        for cb in self.callbacks:
            state = cb.state_dict() if hasattr(cb, "state_dict") else None
            if state:
                ck["callbacks"][getattr(cb, "state_key", type(cb).__qualname__)] = state
        if block is not None:
            ck[R.RESUME_KEY] = block
        tmp = str(path) + ".part"
        torch.save(ck, tmp)
        os.replace(tmp, path)

    def _plan_resume(self, ckpt_path, module, run, rank, world):
        """reads the file (every rank does) and checks everything fit() will restore; ValueError on the first
        thing that does not fit, with no device buffer written yet"""
        import warnings

        from . import resume as R
        ck = torch.load(str(ckpt_path), map_location="cpu", weights_only=True)
        model, opt = module.model, module.optimizer
        arena = model.arena
        block = ck.get(R.RESUME_KEY)
        flat, others = R.plan_weights(model, model.strip_lightning_prefix(ck))
        if block is not None:
            if int(block["version"]) > R.FORMAT_VERSION:
                raise ValueError(f"checkpoint resume block version {block['version']}: this build reads up to "
                                 f"{R.FORMAT_VERSION}")
            diff = R.first_difference(list(block["trainable"]), arena.trainable_names())
            if diff is not None:
                raise ValueError(f"checkpoint optimizer state does not fit the trainable set: {diff}")
        states = ck.get("optimizer_states") or []
        if len(states) != 1:
            raise ValueError(f"checkpoint: {len(states)} optimizer states, this module has one optimizer")
        plan = {"flat": flat, "others": others, "optimizer": opt.plan_load(states[0]), "callbacks": ck.get("callbacks") or {},
                "epoch": int(ck["epoch"]), "global_step": int(ck["global_step"]), "block": block, "grads": None,
                "swa": None, "rng": None, "mid_epoch": False, "skip": 0}
        if block is None:
            warnings.warn(f"Trainer.fit(ckpt_path={str(ckpt_path)!r}): no {R.RESUME_KEY} block (a Lightning / reference "
                          "checkpoint): weights, optimizer state, global_step and epoch are restored; the position "
                          f"inside epoch {plan['epoch']} is not known, its data starts from the beginning",
                          UserWarning, stacklevel=3)
            plan.update(start_epoch=plan["epoch"], micro_step=plan["global_step"] * run.accumulate,
                        runner_global_step=plan["global_step"])
        else:
            micro, acc = int(block["micro_step"]), int(block["accumulate"])
            mid_epoch, mid_window = not block["epoch_finished"], micro % acc != 0
            if mid_epoch or mid_window:
                where = "inside an epoch" if mid_epoch else "inside an accumulation window"
                if int(block["world_size"]) != world:
                    raise ValueError(f"checkpoint taken {where} with world size {block['world_size']}, this run "
                                     f"has {world}")
                if acc != run.accumulate:
                    raise ValueError(f"checkpoint taken {where} with accumulate_grad_batches={acc}, this run has "
                                     f"{run.accumulate}")
            mine = block["ranks"][rank] if rank < len(block["ranks"]) else None
            if mid_window:
                plan["grads"] = arena.join(mine["grads"], "grad", "checkpoint open-window gradients")
            if block.get("swa") is not None:
                plan["swa"] = arena.join(block["swa"], "all", "checkpoint SWA average")
            if mine is not None and int(block["world_size"]) == world:
                plan["rng"] = mine  # (another world size at an epoch boundary: the generators stay as they are)
            plan.update(mid_epoch=mid_epoch, skip=int(block["batches_done"]) if mid_epoch else 0,
                        start_epoch=plan["epoch"] if mid_epoch else plan["epoch"] + 1,
                        micro_step=micro if acc == run.accumulate else int(block["runner_global_step"]) * run.accumulate,
                        runner_global_step=int(block["runner_global_step"]))
        plan["complete"] = (plan["start_epoch"] >= self.max_epochs
                            or (self.max_steps > 0 and plan["global_step"] >= self.max_steps))
        return plan

    def _apply_resume(self, plan, module, run):
        """weights in place (parameter views, compute views and later captures stay valid) + shadow, moments,
        step count and rate, counters, and an open window's partial sums, which the next micro-step adds to"""
        arena = module.model.arena
        with torch.no_grad():
            arena.data.copy_(plan["flat"])
            for own, value in plan["others"]:
                own.copy_(value.to(own.dtype))
            arena.refresh_shadow()
            module.optimizer.apply_load(plan["optimizer"])
            arena.zero_grad()
            if plan["grads"] is not None:
                arena.grad.copy_(plan["grads"])
        self.global_step, self.current_epoch = plan["global_step"], plan["epoch"]
        run.global_step, run.micro_step = plan["runner_global_step"], plan["micro_step"]
        block = plan["block"]
        if block is not None:
            run.seed_base = int(block["seed_base"])
            run.lr_override = None if block["lr_override"] is None else float(block["lr_override"])
            self._batches_done, self._epoch_finished = int(block["batches_done"]), bool(block["epoch_finished"])

    def _restore_callbacks(self, plan, module):
        import warnings
        saved = plan["callbacks"]
        for cb in self.callbacks:
            if not hasattr(cb, "load_state_dict"):
                continue
            key = getattr(cb, "state_key", type(cb).__qualname__)
            if key in saved:
                cb.load_state_dict(saved[key])
            elif cb.state_dict():
                warnings.warn(f"Trainer.fit(ckpt_path=...): the checkpoint has no state for the callback {key}; it "
                              "starts fresh", UserWarning, stacklevel=3)
        arena = module.model.arena
        if plan["swa"] is not None and arena.swa is not None:
            arena.swa.copy_(plan["swa"])

    def _restore_books(self, plan):
        block = plan["block"]
        if block is None:
            return
        self.callback_metrics.clear()
        self.callback_metrics.update(block["callback_metrics"])
        self.history[:] = [dict(r) for r in block["history"]]
        self.val_history[:] = [dict(r) for r in block["val_history"]]


def fit(module: SAM2LightningModule, batches, max_steps: int, device="cuda", log_every: int = 1, distributed=False,
        graph: bool = True, accumulate_grad_batches: int = 1, gradient_clip_val: Optional[float] = 1.0):
    """Minimal fit loop: `max_steps` micro-steps over an iterable of BatchedVideoDatapoint
    (gradient_clip_val 1.0 = best.yaml's trainer section)."""
    module.setup("fit", device)
    run = StepRunner(module, max(1, math.ceil(max_steps / max(1, accumulate_grad_batches))), distributed,
                     graph=graph, accumulate_grad_batches=accumulate_grad_batches,
                     gradient_clip_val=gradient_clip_val)
    hist: List[Dict[str, float]] = []
    t0 = time.time()
    for i, batch in enumerate(batches):
        if i >= max_steps:
            break
        run(_to_device(batch, device))
        if (i + 1) % log_every == 0:
            row = {k: float(v) for k, v in module.logged.items()}
            row["step"] = i + 1
            row["time_s"] = time.time() - t0
            hist.append(row)
    return hist
