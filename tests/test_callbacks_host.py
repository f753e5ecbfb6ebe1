"""The Trainer callbacks without a GPU (sam2_video/training/callbacks.py): ModelCheckpoint, EarlyStopping and
StochasticWeightAveraging against a fake trainer that feeds a scripted metric sequence, the SWA learning rate
against a real torch.optim.swa_utils.SWALR, and the `_target_` resolution of the configs' callbacks."""
import math
import os

import pytest
import torch

from sam2_video.model.build import instantiate
from sam2_video.training import callbacks as C

REF_FILENAME = "sam2-epoch{epoch:02d}-val_loss{val/total_loss:.4f}"  # reference configs/best.yaml:131


class FakeTrainer:
    """what the callbacks ask of a trainer; save_checkpoint writes a small file naming the step"""

    def __init__(self, root, max_epochs=10, base_lr=None):
        self.callback_metrics = {}
        self.current_epoch = 0
        self.global_step = 0
        self.max_epochs = max_epochs
        self.default_root_dir = str(root)
        self.should_stop = False
        self.is_global_zero = True
        self.saved = []
        self.base_lr = base_lr or (lambda epoch: 1e-3)
        self.epoch_lr = None

    def save_checkpoint(self, path):
        self.saved.append(path)
        with open(path, "w") as f:
            f.write(str(self.global_step))

    def current_lr(self):
        return self.epoch_lr if self.epoch_lr is not None else self.base_lr(self.current_epoch)

    def set_epoch_lr(self, lr):
        self.epoch_lr = lr

    def validate(self, cbs, epoch, **metrics):
        self.current_epoch, self.global_step = epoch, 10 * (epoch + 1)
        self.callback_metrics.update({k.replace("__", "/"): v for k, v in metrics.items()})
        for cb in cbs:
            cb.on_validation_end(self, None)


def _files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


SEQ = [0.5, 0.3, 0.4, 0.3, 0.6, 0.1]


def _name(e):
    return f"e{e}.ckpt"


def _run_topk(tmp_path, k, mode="min", seq=SEQ):
    cb = C.ModelCheckpoint(monitor="val/total_loss", mode=mode, save_top_k=k, dirpath=str(tmp_path / "ck"),
                           filename="e{epoch}", auto_insert_metric_name=False)
    tr = FakeTrainer(tmp_path)
    cb.on_fit_start(tr, None)
    seen = []
    for e, v in enumerate(seq):
        tr.validate([cb], e, val__total_loss=v)
        seen.append((_files(tmp_path / "ck") if os.path.isdir(tmp_path / "ck") else [],
                     os.path.basename(cb.best_model_path), cb.best_model_score))
    return cb, tr, seen


def test_top_k_2_keeps_the_two_best_and_deletes_the_one_pushed_out(tmp_path):
    cb, tr, seen = _run_topk(tmp_path, 2)
    # 0.5 | 0.3 | 0.4 pushes e0 out | 0.3 pushes e2 out (a tie with e1: e1 stays the best) | 0.6 does not
    # enter | 0.1 pushes out the k-th best, which of the two 0.3 is the earlier one
    assert [s[0] for s in seen] == [["e0.ckpt"], ["e0.ckpt", "e1.ckpt"], ["e1.ckpt", "e2.ckpt"],
                                    ["e1.ckpt", "e3.ckpt"], ["e1.ckpt", "e3.ckpt"], ["e3.ckpt", "e5.ckpt"]]
    assert [s[1] for s in seen] == ["e0.ckpt", "e1.ckpt", "e1.ckpt", "e1.ckpt", "e1.ckpt", "e5.ckpt"]
    assert [s[2] for s in seen] == [0.5, 0.3, 0.3, 0.3, 0.3, 0.1]
    assert {os.path.basename(p): v for p, v in cb.best_k_models.items()} == {"e3.ckpt": 0.3, "e5.ckpt": 0.1}
    assert os.path.basename(cb.kth_best_model_path) == "e3.ckpt" and cb.kth_value == 0.3
    assert [os.path.basename(p) for p in tr.saved] == [_name(e) for e in (0, 1, 2, 3, 5)]
    assert cb.last_model_path == ""  # save_last was not asked for


def test_top_k_minus_1_keeps_everything(tmp_path):
    cb, tr, seen = _run_topk(tmp_path, -1)
    assert seen[-1][0] == [_name(e) for e in range(6)] and len(cb.best_k_models) == 6
    assert seen[-1][1:] == ("e5.ckpt", 0.1) and seen[3][1] == "e1.ckpt"


def test_top_k_0_saves_nothing(tmp_path):
    cb, tr, seen = _run_topk(tmp_path, 0)
    assert tr.saved == [] and all(s[0] == [] for s in seen)
    assert cb.best_model_path == "" and cb.best_model_score is None and cb.best_k_models == {}


def test_mode_max_and_ties(tmp_path):
    cb, tr, seen = _run_topk(tmp_path, 1, mode="max", seq=[0.2, 0.7, 0.7, 0.1, 0.9])
    assert [s[1] for s in seen] == ["e0.ckpt", "e1.ckpt", "e1.ckpt", "e1.ckpt", "e4.ckpt"]  # the tie keeps e1
    assert seen[-1][0] == ["e4.ckpt"] and cb.best_model_score == 0.9


def test_a_nan_score_never_beats_a_number(tmp_path):
    cb, tr, seen = _run_topk(tmp_path, 1, seq=[float("nan"), 0.4, float("nan")])
    assert [s[1] for s in seen] == ["e0.ckpt", "e1.ckpt", "e1.ckpt"] and seen[-1][0] == ["e1.ckpt"]


def test_reference_filename_nests_a_directory_and_versions_repeat(tmp_path):
    cb = C.ModelCheckpoint(monitor="val/total_loss", mode="min", save_top_k=-1, save_last=True,
                           dirpath=str(tmp_path / "ck"), filename=REF_FILENAME)
    tr = FakeTrainer(tmp_path)
    tr.validate([cb], 2, val__total_loss=0.12341)
    first = os.path.join("sam2-epochepoch=02-val_lossval", "total_loss=0.1234.ckpt")
    assert _files(tmp_path / "ck") == ["last.ckpt", first]
    assert cb.best_model_path == str(tmp_path / "ck" / first)
    tr.validate([cb], 2, val__total_loss=0.12339)  # the same name again
    tr.validate([cb], 2, val__total_loss=0.12342)
    assert _files(tmp_path / "ck") == sorted(["last.ckpt", first, first.replace(".ckpt", "-v1.ckpt"),
                                              first.replace(".ckpt", "-v2.ckpt")])
    assert cb.best_model_path.endswith("-v1.ckpt") and cb.best_model_score == 0.12339
    assert cb.last_model_path == str(tmp_path / "ck" / "last.ckpt")
    assert open(cb.last_model_path).read() == "30"


def test_filename_rules():
    cb = C.ModelCheckpoint(dirpath="d", filename="{epoch}-{step:05d}-{missing:.1f}")
    assert cb.format_checkpoint_name({"epoch": 3, "step": 42}) == os.path.join("d", "epoch=3-step=00042-missing=0.0.ckpt")
    cb = C.ModelCheckpoint(dirpath="d")
    assert cb.format_checkpoint_name({"epoch": 3, "step": 42}, ver=2) == os.path.join("d", "epoch=3-step=42-v2.ckpt")
    cb = C.ModelCheckpoint(dirpath="d", filename="x{val/iou:.2f}", auto_insert_metric_name=False)
    assert cb.format_checkpoint_name({"val/iou": 0.456}) == os.path.join("d", "x0.46.ckpt")


def test_default_dirpath_is_under_the_root_dir(tmp_path):
    cb = C.ModelCheckpoint(monitor="val/total_loss")
    tr = FakeTrainer(tmp_path)
    cb.on_fit_start(tr, None)
    tr.validate([cb], 0, val__total_loss=1.0)
    assert _files(tmp_path) == [os.path.join("checkpoints", "epoch=0-step=10.ckpt")]


def test_a_monitor_that_was_never_logged_raises_at_the_first_validation_end(tmp_path):
    for cb in (C.ModelCheckpoint(monitor="val/nope", dirpath=str(tmp_path)), C.EarlyStopping(monitor="val/nope")):
        tr = FakeTrainer(tmp_path)
        with pytest.raises(RuntimeError, match="val/nope"):
            tr.validate([cb], 0, val__total_loss=1.0)
    assert _files(tmp_path) == []


# ------------------------------------------------------------------------------------------- EarlyStopping
def _stops_at(cb, seq, tmp_path):
    tr = FakeTrainer(tmp_path)
    for e, v in enumerate(seq):
        tr.validate([cb], e, val__total_loss=v)
        if tr.should_stop:
            return e
    return None


@pytest.mark.parametrize("patience", [1, 2, 5])
def test_early_stopping_stops_at_exactly_the_patience_th_bad_check(tmp_path, patience):
    cb = C.EarlyStopping(monitor="val/total_loss", patience=patience, mode="min")
    seq = [1.0, 0.9] + [0.95] * 10
    assert _stops_at(cb, seq, tmp_path) == 1 + patience
    assert cb.wait_count == patience and cb.best_score == 0.9 and cb.stopped_epoch == 1 + patience


def test_early_stopping_an_improvement_resets_the_count(tmp_path):
    cb = C.EarlyStopping(monitor="val/total_loss", patience=2)
    assert _stops_at(cb, [1.0, 1.1, 0.9, 1.0, 0.8, 0.85, 0.81], tmp_path) == 6
    assert cb.best_score == 0.8 and cb.wait_count == 2
    assert _stops_at(C.EarlyStopping(monitor="val/total_loss", patience=3), [1.0, 0.9, 0.8, 0.7], tmp_path) is None


def test_early_stopping_min_delta(tmp_path):
    # improvements of less than min_delta do not count (and do not move best_score)
    cb = C.EarlyStopping(monitor="val/total_loss", patience=2, min_delta=0.1)
    assert _stops_at(cb, [1.0, 0.95, 0.91, 0.5], tmp_path) == 2
    assert cb.best_score == 1.0
    cb = C.EarlyStopping(monitor="val/total_loss", patience=2, min_delta=0.1)
    assert _stops_at(cb, [1.0, 0.95, 0.85, 0.8, 0.76], tmp_path) == 4  # 0.85 < 1.0 - 0.1 counts
    assert cb.best_score == 0.85


def test_early_stopping_mode_max(tmp_path):
    cb = C.EarlyStopping(monitor="val/total_loss", patience=2, mode="max", min_delta=0.05)
    assert _stops_at(cb, [0.1, 0.2, 0.24, 0.3, 0.3, 0.34], tmp_path) == 5
    assert cb.best_score == 0.3


def test_early_stopping_nan_and_check_finite(tmp_path):
    nan = float("nan")
    cb = C.EarlyStopping(monitor="val/total_loss", patience=5)
    assert _stops_at(cb, [1.0, nan, 0.5], tmp_path) == 1 and cb.wait_count == 0
    cb = C.EarlyStopping(monitor="val/total_loss", patience=2, check_finite=False)
    assert _stops_at(cb, [1.0, nan, 0.5, nan, nan], tmp_path) == 4  # a NaN is merely no improvement
    cb = C.EarlyStopping(monitor="val/total_loss", patience=5)
    assert _stops_at(cb, [1.0, math.inf], tmp_path) == 1


def test_early_stopping_thresholds(tmp_path):
    assert _stops_at(C.EarlyStopping(monitor="val/total_loss", stopping_threshold=0.5), [1.0, 0.6, 0.4, 0.3],
                     tmp_path) == 2
    assert _stops_at(C.EarlyStopping(monitor="val/total_loss", divergence_threshold=2.0), [1.0, 1.9, 2.5],
                     tmp_path) == 2


# ---------------------------------------------------------------------------------------------- resolution
def test_config_targets_resolve_to_the_new_classes(tmp_path):
    cb = instantiate({"_target_": "lightning.pytorch.callbacks.ModelCheckpoint", "monitor": "val/total_loss",
                      "mode": "min", "save_top_k": 3, "save_last": True, "dirpath": str(tmp_path),
                      "filename": REF_FILENAME})
    assert type(cb) is C.ModelCheckpoint and cb.save_top_k == 3 and cb.save_last and cb.filename == REF_FILENAME
    cb = instantiate({"_target_": "lightning.pytorch.callbacks.EarlyStopping", "monitor": "val/total_loss",
                      "patience": 5, "mode": "min"})
    assert type(cb) is C.EarlyStopping and cb.patience == 5
    cb = instantiate({"_target_": "lightning.pytorch.callbacks.StochasticWeightAveraging", "swa_lrs": 0.005})
    assert type(cb) is C.StochasticWeightAveraging and cb.swa_lrs == 0.005 and cb.annealing_epochs == 10
    lrm = instantiate({"_target_": "lightning.pytorch.callbacks.LearningRateMonitor", "logging_interval": "step"})
    ms = instantiate({"_target_": "lightning.pytorch.callbacks.ModelSummary", "max_depth": 2})
    assert type(lrm) is C.LearningRateMonitor and type(ms) is C.ModelSummary
    tr = FakeTrainer(tmp_path)
    for cb in (lrm, ms):
        for hook in C.HOOKS:
            getattr(cb, hook)(tr, None)
    assert _files(tmp_path) == [] and not tr.should_stop


def test_trainer_exposes_the_callbacks():
    from sam2_video.training.trainer import Trainer
    ck, es = C.ModelCheckpoint(monitor="val/total_loss"), C.EarlyStopping(monitor="val/total_loss")
    tr = Trainer(max_epochs=2, callbacks=[C.LearningRateMonitor(), ck, C.ModelCheckpoint(), es], default_root_dir="x")
    assert tr.checkpoint_callback is ck and tr.early_stopping_callback is es and tr.default_root_dir == "x"
    assert tr.callback_metrics == {} and tr.should_stop is False
    tr = Trainer(max_epochs=2)
    assert tr.callbacks == [] and tr.checkpoint_callback is None and tr.early_stopping_callback is None


# ---------------------------------------------------------------------------------------------------- SWA
class FakeArena:
    def __init__(self):
        self.calls = []

    def swa_buffer(self):
        self.calls.append("buffer")

    def swa_update(self, n_averaged):
        self.calls.append(("update", n_averaged))

    def swa_apply(self):
        self.calls.append("apply")


class FakeModule:
    def __init__(self, extra=None):
        self.model = torch.nn.Sequential(torch.nn.Linear(2, 2), *([extra] if extra is not None else []))
        self.model.arena = FakeArena()


def _swalr_rates(base_lr, swa_lr, anneal_epochs, strategy, max_epochs, epochs):
    """the rate of each of `epochs` epochs under a real SWALR built as the callback's specification says"""
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=base_lr)
    for g in opt.param_groups:
        g["initial_lr"] = swa_lr
    sched = torch.optim.swa_utils.SWALR(opt, swa_lr=swa_lr, anneal_epochs=anneal_epochs, anneal_strategy=strategy,
                                        last_epoch=max_epochs if strategy == "linear" else -1)
    rates = []
    for _ in range(epochs):
        rates.append(opt.param_groups[0]["lr"])
        opt.step()
        sched.step()
    return rates


@pytest.mark.parametrize("strategy", ["cos", "linear"])
@pytest.mark.parametrize("anneal_epochs", [1, 3, 10])
def test_swa_learning_rate_is_swalr(tmp_path, strategy, anneal_epochs):
    max_epochs, start = 14, 2

    def base(epoch):  # what the per-step schedule would give at each epoch's start
        return 1e-3 * (0.5 + 0.5 * math.cos(math.pi * epoch / max_epochs))

    cb = C.StochasticWeightAveraging(swa_lrs=0.005, swa_epoch_start=start, annealing_epochs=anneal_epochs,
                                     annealing_strategy=strategy)
    tr, mod = FakeTrainer(tmp_path, max_epochs=max_epochs, base_lr=base), FakeModule()
    cb.on_fit_start(tr, mod)
    assert (cb.swa_start, cb.swa_end) == (1, 13)
    got = []
    for e in range(max_epochs):
        tr.current_epoch = e
        cb.on_train_epoch_start(tr, mod)
        got.append(tr.current_lr())
        cb.on_train_epoch_end(tr, mod)
    cb.on_train_end(tr, mod)
    assert got[0] == base(0) and tr.epoch_lr is not None
    want = _swalr_rates(base(1), 0.005, anneal_epochs, strategy, max_epochs, max_epochs - 1)
    assert want[0] == base(1) and abs(want[-1] - 0.005) <= 1e-9 * 0.005
    for e, (a, b) in enumerate(zip(got[1:], want)):
        assert abs(a - b) <= 1e-9 * abs(b), (e + 1, a, b)
    assert mod.model.arena.calls == ["buffer"] + [("update", n) for n in range(13)] + ["apply"]


@pytest.mark.parametrize("max_epochs,float_range,int_range", [(1, (0, 0), (1, 0)), (3, (1, 2), (1, 2)),
                                                              (5, (3, 4), (1, 4)), (10, (7, 9), (1, 9))])
def test_swa_epoch_range(tmp_path, max_epochs, float_range, int_range):
    for start, want in ((0.8, float_range), (2, int_range)):
        cb = C.StochasticWeightAveraging(swa_lrs=0.005, swa_epoch_start=start)
        tr, mod = FakeTrainer(tmp_path, max_epochs=max_epochs), FakeModule()
        cb.on_fit_start(tr, mod)
        assert (cb.swa_start, cb.swa_end) == want == cb.epoch_range(max_epochs)
        for e in range(max_epochs):
            tr.current_epoch = e
            cb.on_train_epoch_start(tr, mod)
            cb.on_train_epoch_end(tr, mod)
        cb.on_train_end(tr, mod)
        n = max(0, want[1] - want[0] + 1)
        updates = [c for c in mod.model.arena.calls if c != "buffer"]
        assert updates == [("update", k) for k in range(n)] + (["apply"] if n else [])


def test_swa_is_not_applied_when_the_run_stops_before_swa_end(tmp_path):
    cb = C.StochasticWeightAveraging(swa_lrs=0.005, swa_epoch_start=0.5)
    tr, mod = FakeTrainer(tmp_path, max_epochs=6), FakeModule()
    cb.on_fit_start(tr, mod)
    for e in range(4):  # an early stop after epoch 3; swa_end is 5
        tr.current_epoch = e
        cb.on_train_epoch_start(tr, mod)
        cb.on_train_epoch_end(tr, mod)
    cb.on_train_end(tr, mod)
    assert mod.model.arena.calls == ["buffer", ("update", 0), ("update", 1)]


def test_swa_argument_checks(tmp_path):
    with pytest.raises(NotImplementedError):
        C.StochasticWeightAveraging(swa_lrs=0.005, avg_fn=lambda a, p, n: a)
    with pytest.raises(TypeError):
        C.StochasticWeightAveraging()
    for bad in (dict(swa_lrs=0.0), dict(swa_lrs=[0.1]), dict(swa_lrs=0.1, annealing_strategy="exp"),
                dict(swa_lrs=0.1, swa_epoch_start=0), dict(swa_lrs=0.1, swa_epoch_start=1.5),
                dict(swa_lrs=0.1, annealing_epochs=-1)):
        with pytest.raises(ValueError):
            C.StochasticWeightAveraging(**bad)
    cb = C.StochasticWeightAveraging(swa_lrs=0.005)
    with pytest.raises(NotImplementedError, match="BatchNorm"):
        cb.on_fit_start(FakeTrainer(tmp_path), FakeModule(torch.nn.BatchNorm1d(2)))
