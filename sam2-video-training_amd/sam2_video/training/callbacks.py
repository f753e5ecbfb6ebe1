"""The Lightning callbacks the reference configs name, for this build's Trainer (training/trainer.py) when
Lightning is not installed: ModelCheckpoint, EarlyStopping, StochasticWeightAveraging, and the two that only
log (LearningRateMonitor, ModelSummary), which take their arguments and do nothing.  `model/build.py` resolves
`lightning.pytorch.callbacks.*` to these classes when Lightning cannot be imported; under a real
`lightning.pytorch.Trainer` Lightning's own callbacks run and nothing here is used.

The behaviour follows the rules of Lightning 2.x as the project's DESIGN.md §9 states them; they were written
down from Lightning's documented behaviour and were not compared with Lightning itself (it is not installed).

What a trainer must offer (this build's Trainer does; tests drive the callbacks with a small fake):
`callback_metrics` (name -> float), `current_epoch`, `global_step`, `max_epochs`, `default_root_dir`,
`should_stop`, `is_global_zero`, `save_checkpoint(path)`, and for StochasticWeightAveraging `current_lr()` /
`set_epoch_lr(lr)`.  Hooks have Lightning's signature `hook(trainer, pl_module)`.  A callback's `state_dict()`
goes into every checkpoint under its `state_key`; a resumed fit hands it to `load_state_dict` after on_fit_start.
"""
from __future__ import annotations

import math
import os
import re
from typing import Dict, Optional

HOOKS = ("on_fit_start", "on_train_epoch_start", "on_validation_end", "on_train_epoch_end", "on_train_end")


class Callback:
    """base class: every hook the Trainer calls, as a no-op"""

    def on_fit_start(self, trainer, pl_module):
        pass

    def on_train_epoch_start(self, trainer, pl_module):
        pass

    def on_validation_end(self, trainer, pl_module):
        pass

    def on_train_epoch_end(self, trainer, pl_module):
        pass

    def on_train_end(self, trainer, pl_module):
        pass

    # ---- state in a checkpoint (Trainer.save_checkpoint writes {state_key: state_dict()} of every callback
    # whose state is not empty; a resumed fit calls load_state_dict after on_fit_start)
    @property
    def state_key(self) -> str:
        """what the state is filed under: the class name, plus the arguments that tell two callbacks of a
        class apart (_state_key)"""
        return type(self).__qualname__

    @staticmethod
    def _state_key(cls_name: str, **kw) -> str:
        return f"{cls_name}{kw!r}"

    def state_dict(self) -> dict:
        """numbers, strings, lists and dicts only (the file loads with weights_only=True)"""
        return {}

    def load_state_dict(self, state: dict):
        pass


class LearningRateMonitor(Callback):
    """accepted and inert: the Trainer's history rows already carry train/learning_rate"""

    def __init__(self, logging_interval=None, log_momentum=False, log_weight_decay=False):
        self.logging_interval = logging_interval
        self.log_momentum = log_momentum
        self.log_weight_decay = log_weight_decay


class ModelSummary(Callback):
    """accepted and inert"""

    def __init__(self, max_depth: int = 1, **summarize_kwargs):
        self.max_depth = max_depth


def _mode_ops(mode: str):
    if mode not in ("min", "max"):
        raise ValueError(f"mode must be 'min' or 'max', got {mode!r}")
    return (lambda a, b: a < b) if mode == "min" else (lambda a, b: a > b)


def _monitored(trainer, monitor: str, who: str) -> float:
    metrics = trainer.callback_metrics
    if monitor not in metrics:
        raise RuntimeError(f"{who}(monitor={monitor!r}): the metric was never logged; available: "
                           f"{sorted(metrics)}")
    return float(metrics[monitor])


class ModelCheckpoint(Callback):
    """Saves through `trainer.save_checkpoint` at each validation end, keeps the `save_top_k` best by the
    monitored score (-1: all, 0: none) and deletes the one pushed out; `save_last` also writes `last.ckpt`.
    A score must beat the current k-th best strictly to enter a full list, so of two equal scores the earlier
    checkpoint stays and `best_model_path` names the earliest of the best."""

    CHECKPOINT_NAME_LAST = "last"
    FILE_EXTENSION = ".ckpt"

    def __init__(self, dirpath=None, filename=None, monitor=None, verbose=False, save_last=None, save_top_k=1,
                 save_weights_only=False, mode="min", auto_insert_metric_name=True, **unused):
        self.dirpath = None if dirpath is None else str(dirpath)
        self.filename = filename
        self.monitor = monitor
        self.save_last = bool(save_last)
        self.save_top_k = int(save_top_k)
        if self.save_top_k < -1:
            raise ValueError(f"save_top_k={save_top_k}: -1 (all), 0 (none) or a positive count")
        if monitor is None and self.save_top_k not in (-1, 0, 1):
            raise ValueError(f"save_top_k={save_top_k} needs a monitor")
        self.mode = mode
        self._better = _mode_ops(mode)
        self.auto_insert_metric_name = bool(auto_insert_metric_name)
        self.best_k_models: Dict[str, float] = {}
        self.kth_best_model_path = ""
        self.kth_value = math.inf if mode == "min" else -math.inf
        self.best_model_path = ""
        self.best_model_score: Optional[float] = None
        self.last_model_path = ""
        self.current_score: Optional[float] = None  # the monitored value of the latest validation

    # ---- names
    def format_checkpoint_name(self, metrics: Dict[str, float], ver: Optional[int] = None) -> str:
        """each `{name[:fmt]}` of `filename` becomes `name=<value>` (just `<value>` without
        auto_insert_metric_name); a metric that is not there formats as 0; `-v<ver>` is appended"""
        filename = self.filename if self.filename is not None else "{epoch}-{step}"
        for group in re.findall(r"(\{.*?)[:\}]", filename):
            name = group[1:]
            if self.auto_insert_metric_name:
                filename = filename.replace(group, name + "={" + name)
            filename = filename.replace("{" + name, "{0[" + name + "]")
            if name not in metrics:
                metrics = dict(metrics, **{name: 0})
        filename = filename.format(metrics)
        if ver is not None:
            filename = f"{filename}-v{ver}"
        return os.path.join(self.dirpath, filename + self.FILE_EXTENSION) if self.dirpath else filename + self.FILE_EXTENSION

    def _candidates(self, trainer) -> Dict[str, float]:
        m = dict(trainer.callback_metrics)
        m["epoch"] = int(trainer.current_epoch)
        m["step"] = int(trainer.global_step)
        return m

    def _fresh_path(self, metrics, del_path=None) -> str:
        path = self.format_checkpoint_name(metrics)
        ver = 1
        while os.path.exists(path) and path != del_path:
            path = self.format_checkpoint_name(metrics, ver=ver)
            ver += 1
        return path

    # ---- files (rank 0 writes and deletes; every rank keeps the same books)
    def _save(self, trainer, path):
        if getattr(trainer, "is_global_zero", True):
            os.makedirs(os.path.dirname(path) or ".", exist_ok=True)  # a metric named a/b nests a directory
        trainer.save_checkpoint(path)

    @staticmethod
    def _remove(trainer, path):
        if getattr(trainer, "is_global_zero", True) and os.path.isfile(path):
            os.remove(path)

    # ---- hooks
    def on_fit_start(self, trainer, pl_module):
        if self.dirpath is None:
            root = getattr(trainer, "default_root_dir", None) or os.getcwd()
            self.dirpath = os.path.join(str(root), "checkpoints")

    def on_validation_end(self, trainer, pl_module):
        if self.dirpath is None:
            self.on_fit_start(trainer, pl_module)
        metrics = self._candidates(trainer)
        if self.monitor is not None:
            current = _monitored(trainer, self.monitor, "ModelCheckpoint")
            self.current_score = current
            if self.save_top_k != 0:
                if math.isnan(current):
                    current = math.inf if self.mode == "min" else -math.inf
                if self._enters_top_k(current):
                    self._update_best_and_save(current, trainer, metrics)
        elif self.save_top_k != 0:
            # no monitor: the latest checkpoint (save_top_k 1 replaces it, -1 keeps every one)
            previous = self.best_model_path
            path = self._fresh_path(metrics, previous if self.save_top_k == 1 else None)
            self.best_model_path = path
            self._save(trainer, path)
            if self.save_top_k == 1 and previous and previous != path:
                self._remove(trainer, previous)
        if self.save_last:
            path = os.path.join(self.dirpath, self.CHECKPOINT_NAME_LAST + self.FILE_EXTENSION)
            previous, self.last_model_path = self.last_model_path, path
            self._save(trainer, path)
            if previous and previous != path:
                self._remove(trainer, previous)

    # ---- state
    @property
    def state_key(self) -> str:
        return self._state_key(type(self).__qualname__, monitor=self.monitor, mode=self.mode, filename=self.filename)

    def state_dict(self) -> dict:
        return {"monitor": self.monitor, "best_model_score": self.best_model_score,
                "best_model_path": self.best_model_path, "current_score": self.current_score,
                "dirpath": self.dirpath, "best_k_models": dict(self.best_k_models),
                "kth_best_model_path": self.kth_best_model_path, "kth_value": self.kth_value,
                "last_model_path": self.last_model_path}

    def load_state_dict(self, state: dict):
        """the top-k books describe files in `dirpath`: they are taken over when the resumed run writes to the
        same directory; with another one only best_model_path is (and a warning says so), and the new
        directory starts its own list"""
        saved_dir = state.get("dirpath", self.dirpath)
        if self.dirpath == saved_dir:
            self.best_model_score = state["best_model_score"]
            self.kth_best_model_path = state.get("kth_best_model_path", self.kth_best_model_path)
            self.kth_value = state.get("kth_value", self.kth_value)
            self.best_k_models = dict(state.get("best_k_models", self.best_k_models))
            self.last_model_path = state.get("last_model_path", self.last_model_path)
            self.current_score = state.get("current_score", self.current_score)
        else:
            import warnings
            warnings.warn(f"ModelCheckpoint: the checkpoint was written with dirpath={saved_dir!r}, this run uses "
                          f"{self.dirpath!r}: best_model_score, best_k_models, kth_* and last_model_path are not "
                          "restored", UserWarning, stacklevel=2)
        self.best_model_path = state["best_model_path"]

    def _enters_top_k(self, current: float) -> bool:
        if self.save_top_k == -1 or len(self.best_k_models) < self.save_top_k:
            return True
        return self._better(current, self.best_k_models[self.kth_best_model_path])

    def _update_best_and_save(self, current, trainer, metrics):
        k = len(self.best_k_models) + 1 if self.save_top_k == -1 else self.save_top_k
        del_path = None
        if len(self.best_k_models) == k and k > 0:
            del_path = self.kth_best_model_path
            self.best_k_models.pop(del_path)
        path = self._fresh_path(metrics, del_path)
        self.best_k_models[path] = current
        pick_worst, pick_best = (max, min) if self.mode == "min" else (min, max)
        if len(self.best_k_models) == k:
            self.kth_best_model_path = pick_worst(self.best_k_models, key=self.best_k_models.get)
            self.kth_value = self.best_k_models[self.kth_best_model_path]
        self.best_model_path = pick_best(self.best_k_models, key=self.best_k_models.get)  # the earliest on a tie
        self.best_model_score = self.best_k_models[self.best_model_path]
        self._save(trainer, path)
        if del_path is not None and del_path != path:
            self._remove(trainer, del_path)


class EarlyStopping(Callback):
    """Checked at each validation end: an improvement is `current < best_score - min_delta` (mode min; mirrored
    for max) and resets `wait_count`; anything else counts, and `wait_count >= patience` sets
    `trainer.should_stop`.  check_finite stops on a NaN / infinite value, stopping_threshold once the value is
    better than it, divergence_threshold once it is worse."""

    def __init__(self, monitor, min_delta=0.0, patience=3, verbose=False, mode="min", strict=True, check_finite=True,
                 stopping_threshold=None, divergence_threshold=None, **unused):
        self.monitor = monitor
        self.min_delta = abs(float(min_delta))
        self.patience = int(patience)
        self.mode = mode
        self._better = _mode_ops(mode)
        self.check_finite = bool(check_finite)
        self.stopping_threshold = stopping_threshold
        self.divergence_threshold = divergence_threshold
        self.best_score = math.inf if mode == "min" else -math.inf
        self.wait_count = 0
        self.stopped_epoch = 0
        self.reason: Optional[str] = None

    @property
    def state_key(self) -> str:
        return self._state_key(type(self).__qualname__, monitor=self.monitor, mode=self.mode)

    def state_dict(self) -> dict:
        return {"wait_count": self.wait_count, "stopped_epoch": self.stopped_epoch, "best_score": self.best_score,
                "patience": self.patience}

    def load_state_dict(self, state: dict):
        self.wait_count = int(state["wait_count"])
        self.stopped_epoch = int(state["stopped_epoch"])
        self.best_score = float(state["best_score"])
        self.patience = int(state["patience"])

    def _improved(self, current: float) -> bool:
        if self.mode == "min":
            return current < self.best_score - self.min_delta
        return current > self.best_score + self.min_delta

    def on_validation_end(self, trainer, pl_module):
        current = _monitored(trainer, self.monitor, "EarlyStopping")
        stop = False
        if self.check_finite and not math.isfinite(current):
            stop, self.reason = True, f"{self.monitor} = {current} is not finite"
        elif self.stopping_threshold is not None and self._better(current, float(self.stopping_threshold)):
            stop, self.reason = True, f"{self.monitor} = {current} passed the stopping threshold"
        elif self.divergence_threshold is not None and self._better(float(self.divergence_threshold), current):
            stop, self.reason = True, f"{self.monitor} = {current} passed the divergence threshold"
        elif self._improved(current):
            self.best_score = current
            self.wait_count = 0
        else:
            self.wait_count += 1
            if self.wait_count >= self.patience:
                stop, self.reason = True, f"{self.monitor} did not improve in the last {self.wait_count} checks"
        if stop:
            trainer.should_stop = True
            self.stopped_epoch = int(trainer.current_epoch)


class SWALRSchedule:
    """`torch.optim.swa_utils.SWALR` for one learning rate, in Python doubles and with SWALR's own recursion
    (each step undoes the previous interpolation of the CURRENT rate and applies the next one), built on the
    rate the optimizer holds at that moment.  `lr` is the rate of the current epoch; `step()` is SWALR.step(),
    called once per epoch end.  SWALR's last_epoch does not enter its rates."""

    def __init__(self, lr: float, swa_lr: float, anneal_epochs: int = 10, anneal_strategy: str = "cos"):
        if anneal_strategy not in ("cos", "linear"):
            raise ValueError(f"annealing_strategy must be 'cos' or 'linear', got {anneal_strategy!r}")
        if not isinstance(anneal_epochs, int) or anneal_epochs < 0:
            raise ValueError(f"annealing_epochs must be a non-negative integer, got {anneal_epochs!r}")
        self.lr = float(lr)
        self.swa_lr = float(swa_lr)
        self.anneal_epochs = anneal_epochs
        self.anneal_strategy = anneal_strategy
        self._step_count = 1  # SWALR's constructor takes the initial step, which leaves the rate as it is

    def _alpha(self, t: float) -> float:
        return (1 - math.cos(math.pi * t)) / 2 if self.anneal_strategy == "cos" else t

    def state_dict(self) -> dict:
        return {"lr": self.lr, "swa_lr": self.swa_lr, "anneal_epochs": self.anneal_epochs,
                "anneal_strategy": self.anneal_strategy, "_step_count": self._step_count}

    @classmethod
    def from_state(cls, state: dict) -> "SWALRSchedule":
        sched = cls(state["lr"], state["swa_lr"], int(state["anneal_epochs"]), state["anneal_strategy"])
        sched._step_count = int(state["_step_count"])
        return sched

    def step(self) -> float:
        self._step_count += 1
        step = self._step_count - 1
        if self.anneal_epochs == 0:
            step = max(1, step)
        prev_t = max(0, min(1, (step - 1) / max(1, self.anneal_epochs)))
        prev_alpha = self._alpha(prev_t)
        prev_lr = self.swa_lr if prev_alpha == 1 else (self.lr - prev_alpha * self.swa_lr) / (1 - prev_alpha)
        t = max(0, min(1, step / max(1, self.anneal_epochs)))
        alpha = self._alpha(t)
        self.lr = self.swa_lr * alpha + prev_lr * (1 - alpha)
        return self.lr


class StochasticWeightAveraging(Callback):
    """Averages the weights of the epochs [swa_start, swa_end] in one pass over the flat parameter arena per
    epoch (kernels/arena.py swa_update: s2h_swa_update) and, from swa_start on, replaces the per-step schedule
    by SWALRSchedule's rate, constant within an epoch.  At the end of a run that reached swa_end the average is
    written into the master arena and its bf16 shadow in place (s2h_swa_apply): parameter views and captured
    step graphs stay valid, the optimizer moments are untouched.  The model has no BatchNorm, so Lightning's
    extra statistics epoch does not exist; a BatchNorm in the model raises."""

    def __init__(self, swa_lrs, swa_epoch_start=0.8, annealing_epochs: int = 10, annealing_strategy: str = "cos",
                 avg_fn=None, device=None):
        if avg_fn is not None:
            raise NotImplementedError("StochasticWeightAveraging(avg_fn=...): only the default running mean is "
                                      "built (one kernel over the parameter arena)")
        if isinstance(swa_lrs, bool) or not isinstance(swa_lrs, (int, float)) or not swa_lrs > 0:
            raise ValueError(f"swa_lrs must be a positive float, got {swa_lrs!r}")
        if isinstance(swa_epoch_start, bool) or not isinstance(swa_epoch_start, (int, float)):
            raise ValueError(f"swa_epoch_start must be an int or a float, got {swa_epoch_start!r}")
        if isinstance(swa_epoch_start, int) and swa_epoch_start < 1:
            raise ValueError("swa_epoch_start as an int must be >= 1")
        if isinstance(swa_epoch_start, float) and not 0 <= swa_epoch_start <= 1:
            raise ValueError("swa_epoch_start as a float must be in [0, 1]")
        SWALRSchedule(1.0, swa_lrs, annealing_epochs, annealing_strategy)  # validates the two arguments
        self.swa_lrs = float(swa_lrs)
        self.swa_epoch_start = swa_epoch_start
        self.annealing_epochs = annealing_epochs
        self.annealing_strategy = annealing_strategy
        self.swa_start: Optional[int] = None
        self.swa_end: Optional[int] = None
        self.n_averaged = 0
        self.schedule: Optional[SWALRSchedule] = None
        self._latest_update_epoch = -1
        self.applied = False

    def epoch_range(self, max_epochs: int):
        """(swa_start, swa_end): a float start is int(max_epochs * f); the averaging starts one epoch before it"""
        start = self.swa_epoch_start
        if isinstance(start, float):
            start = int(max_epochs * start)
        return max(start - 1, 0), max_epochs - 1

    @staticmethod
    def _arena(pl_module):
        return pl_module.model.arena

    def on_fit_start(self, trainer, pl_module):
        import torch
        model = getattr(pl_module, "model", None)
        if model is not None and any(isinstance(m, torch.nn.modules.batchnorm._BatchNorm) for m in model.modules()):
            raise NotImplementedError("StochasticWeightAveraging: the model has a BatchNorm layer; the extra epoch "
                                      "that recomputes its statistics is not built")
        self.swa_start, self.swa_end = self.epoch_range(int(trainer.max_epochs))
        if model is not None and self.swa_start <= self.swa_end:
            self._arena(pl_module).swa_buffer()  # allocated now, before any step graph is captured

    def on_train_epoch_start(self, trainer, pl_module):
        epoch = int(trainer.current_epoch)
        if self.swa_start is None:
            self.on_fit_start(trainer, pl_module)
        if self.schedule is None and self.swa_start <= epoch <= self.swa_end:
            self.schedule = SWALRSchedule(trainer.current_lr(), self.swa_lrs, self.annealing_epochs,
                                          self.annealing_strategy)
            trainer.set_epoch_lr(self.schedule.lr)
        if self.swa_start <= epoch <= self.swa_end and epoch > self._latest_update_epoch:
            self._arena(pl_module).swa_update(self.n_averaged)
            self.n_averaged += 1
            self._latest_update_epoch = epoch

    def on_train_epoch_end(self, trainer, pl_module):
        if self.schedule is not None:
            trainer.set_epoch_lr(self.schedule.step())

    def state_dict(self) -> dict:
        """the counters and the SWA schedule's position; the average itself (`arena.swa`) is a tensor of the
        checkpoint's own block, written per parameter name by Trainer.save_checkpoint"""
        return {"n_averaged": self.n_averaged, "_latest_update_epoch": self._latest_update_epoch,
                "applied": self.applied, "schedule": None if self.schedule is None else self.schedule.state_dict()}

    def load_state_dict(self, state: dict):
        """after on_fit_start: swa_start / swa_end stay this run's own (a larger max_epochs moves swa_end)"""
        self.n_averaged = int(state["n_averaged"])
        self._latest_update_epoch = int(state["_latest_update_epoch"])
        self.applied = bool(state["applied"])
        self.schedule = None if state.get("schedule") is None else SWALRSchedule.from_state(state["schedule"])

    def on_train_end(self, trainer, pl_module):
        if self.n_averaged > 0 and self._latest_update_epoch == self.swa_end and not self.applied:
            self._arena(pl_module).swa_apply()
            self.applied = True
