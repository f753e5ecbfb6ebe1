"""The Trainer's callbacks, arena SWA and the post-training evaluation block on the device.

One fit (module fixture): Hiera-T 256^2 of tests/golden/overfit_cfg1.json, 2-frame synthetic clips, 2 train clips
and 1 val clip, max_epochs 5, captured step graph, ModelCheckpoint(save_top_k=2, save_last) and
StochasticWeightAveraging(swa_epoch_start=0.6, annealing_epochs=2): swa_start = int(5 * 0.6) - 1 = 2, swa_end = 4.
A recording callback snapshots the master arena at every epoch start and the learning rate at every epoch end.
A second fit stops early on a monitor forced not to improve.  main([...]) runs the post-training block on a tiny
on-disk COCO clip."""
import copy
import json
import os

import numpy as np
import pytest
import torch

from step_harness import GOLD

pytestmark = pytest.mark.gpu

CFG = os.path.join(GOLD, "overfit_cfg1.json")
REF_FILENAME = "sam2-epoch{epoch:02d}-val_loss{val/total_loss:.4f}"
SWA_LR, MAX_EPOCHS = 0.005, 5


def _sections():
    with open(CFG) as f:
        cfg = json.load(f)
    cfg = copy.deepcopy(cfg)
    for model in (cfg["model"], cfg["module"]["model"]):
        model["use_activation_checkpoint"] = False  # (a no-recompute notice otherwise)
    for data in (cfg["data"], cfg["data_module"]["data"]):
        data.update(video_clip_length=2, num_workers=0, synthetic_clips=2)
    return cfg


def _module_and_data(cfg):
    from sam2_video.model.build import instantiate
    return instantiate(cfg["module"], _recursive_=False), instantiate(cfg["data_module"], _recursive_=False)


class Recorder:
    """snapshots for the assertions below (a callback needs only the hooks it uses)"""

    def __init__(self):
        self.start_data, self.start_lr, self.start_step, self.end_lr, self.val_live, self.hooks = {}, {}, {}, {}, {}, []

    def on_fit_start(self, trainer, pl_module):
        self.hooks.append("fit_start")
        self.name = pl_module.model.arena.grad_names[0]

    def on_train_epoch_start(self, trainer, pl_module):
        e = trainer.current_epoch
        self.hooks.append(("epoch_start", e))
        self.start_lr[e], self.start_step[e] = trainer.current_lr(), trainer.global_step
        if e >= 2:
            self.start_data[e] = pl_module.model.arena.data.cpu().clone()

    def on_validation_end(self, trainer, pl_module):
        self.hooks.append(("validation_end", trainer.current_epoch))
        self.val_live[trainer.current_epoch] = pl_module.model.get_parameter(self.name).detach().cpu().clone()
        self.metrics = dict(trainer.callback_metrics)

    def on_train_epoch_end(self, trainer, pl_module):
        self.hooks.append(("epoch_end", trainer.current_epoch))
        self.end_lr[trainer.current_epoch] = pl_module.optimizer.param_groups[0]["lr"]

    def on_train_end(self, trainer, pl_module):
        self.hooks.append("train_end")


@pytest.fixture(scope="module")
def fitted(tmp_path_factory):
    from sam2_video.training import callbacks as C
    from sam2_video.training.trainer import Trainer
    root = tmp_path_factory.mktemp("fit")
    module, dm = _module_and_data(_sections())
    rec = Recorder()
    ck = C.ModelCheckpoint(monitor="val/total_loss", mode="min", save_top_k=2, save_last=True,
                           dirpath=str(root / "checkpoints"), filename=REF_FILENAME)
    swa = C.StochasticWeightAveraging(swa_lrs=SWA_LR, swa_epoch_start=0.6, annealing_epochs=2)
    trainer = Trainer(max_epochs=MAX_EPOCHS, precision=16, gradient_clip_val=1.0, limit_val_batches=1,
                      val_check_interval=1.0, log_every_n_steps=1, graph=True, num_sanity_val_steps=1,
                      callbacks=[rec, C.LearningRateMonitor(), ck, swa], default_root_dir=str(root / "logs"))
    trainer.fit(module, dm)
    torch.cuda.synchronize()
    return {"trainer": trainer, "module": module, "rec": rec, "ck": ck, "swa": swa, "root": root}


def test_hooks_fire_in_order_and_metrics_are_floats(fitted):
    rec, tr = fitted["rec"], fitted["trainer"]
    want = ["fit_start"]
    for e in range(MAX_EPOCHS):
        want += [("epoch_start", e), ("validation_end", e), ("epoch_end", e)]
    assert rec.hooks == want + ["train_end"]  # (the sanity validation triggered nothing)
    assert tr.global_step == 10 and len(tr.val_history) == MAX_EPOCHS and not tr.should_stop
    assert tr.checkpoint_callback is fitted["ck"] and tr.early_stopping_callback is None
    m = tr.callback_metrics
    assert {"val/total_loss", "val/iou", "train/total_loss", "train/learning_rate"} <= set(m)
    assert all(type(v) is float for v in m.values())
    assert m["val/total_loss"] == tr.val_history[-1]["val/total_loss"]
    assert 1 <= len(tr.runner._graphs) <= 2  # one captured graph per clip layout served the whole run


def test_final_master_is_the_running_average_of_the_swa_epochs(fitted):
    rec, swa, arena = fitted["rec"], fitted["swa"], fitted["module"].model.arena
    assert (swa.swa_start, swa.swa_end, swa.n_averaged, swa.applied) == (2, 4, 3, True)
    assert sorted(rec.start_data) == [2, 3, 4]
    want = rec.start_data[2].clone()
    for k, e in ((1, 3), (2, 4)):
        want = want + (rec.start_data[e] - want) / torch.tensor(k + 1)
    assert not torch.equal(rec.start_data[3], rec.start_data[2]) and not torch.equal(want, rec.start_data[4])
    assert torch.equal(arena.data.cpu(), want)
    assert torch.equal(arena.swa.cpu(), want)
    from sam2_video.kernels import ops
    assert arena.shadow is not None and torch.equal(arena.shadow, ops.cast(arena.data, torch.bfloat16))
    p = fitted["module"].model.get_parameter(rec.name)  # the parameters are views: they show the average
    o = arena.offsets[rec.name]
    assert torch.equal(p.detach().cpu().reshape(-1), want[o:o + p.numel()])


def test_learning_rate_of_the_swa_epochs_is_swalr(fitted):
    rec, module = fitted["rec"], fitted["module"]
    # epochs 0 and 1 follow the per-step schedule; epoch 2 keeps the rate the optimizer held at its start
    assert rec.start_step == {e: 2 * e for e in range(MAX_EPOCHS)}
    assert rec.end_lr[0] == module.lr_at(1) and rec.end_lr[1] == module.lr_at(3)
    base = module.lr_at(4)
    assert rec.start_lr[2] == base and 0 < base < 1e-4
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=base)
    opt.param_groups[0]["initial_lr"] = SWA_LR
    sched = torch.optim.swa_utils.SWALR(opt, swa_lr=SWA_LR, anneal_epochs=2, anneal_strategy="cos")
    for e in (2, 3, 4):
        want = opt.param_groups[0]["lr"]
        assert abs(rec.end_lr[e] - want) <= 1e-9 * want, (e, rec.end_lr[e], want)
        assert abs(rec.start_lr[e] - want) <= 1e-9 * want
        opt.step()
        sched.step()
    assert abs(rec.end_lr[4] - SWA_LR) <= 1e-9 * SWA_LR and rec.end_lr[3] > rec.end_lr[2]


def test_two_ranked_checkpoints_and_last(fitted):
    ck, tr, rec, root = fitted["ck"], fitted["trainer"], fitted["rec"], fitted["root"]
    files = sorted(os.path.relpath(os.path.join(d, f), root / "checkpoints")
                   for d, _, fs in os.walk(root / "checkpoints") for f in fs)
    ranked = sorted(os.path.relpath(p, root / "checkpoints") for p in ck.best_k_models)
    assert len(ranked) == 2 and files == sorted(ranked + ["last.ckpt"])
    assert all(f.startswith("sam2-epochepoch=0") and "/total_loss=" in f for f in ranked)
    losses = [row["val/total_loss"] for row in tr.val_history]
    assert sorted(ck.best_k_models.values()) == sorted(losses)[:2]
    assert ck.best_model_score == min(losses) and ck.best_k_models[ck.best_model_path] == min(losses)
    best = torch.load(ck.best_model_path, map_location="cpu", weights_only=False)
    assert best["state_dict"] and all(k.startswith("model.") for k in best["state_dict"])
    assert best["epoch"] == losses.index(min(losses)) and best["global_step"] == 2 * (best["epoch"] + 1)
    assert set(best["state_dict"]) == {"model." + k for k in fitted["module"].model.state_dict()}
    # a checkpoint written during the SWA phase holds the live weights, not the average
    last = torch.load(ck.last_model_path, map_location="cpu", weights_only=False)
    assert last["epoch"] == 4
    assert torch.equal(last["state_dict"]["model." + rec.name], rec.val_live[4])
    now = fitted["module"].model.get_parameter(rec.name).detach().cpu()
    assert not torch.equal(now, rec.val_live[4])


class ForcedMonitor:
    """logs a monitor that never improves"""

    def on_validation_end(self, trainer, pl_module):
        trainer.callback_metrics["val/forced"] = 1.0


def test_early_stopping_leaves_after_the_second_validation(tmp_path):
    from sam2_video.training import callbacks as C
    from sam2_video.training.trainer import Trainer
    module, dm = _module_and_data(_sections())
    es = C.EarlyStopping(monitor="val/forced", patience=1, mode="min")
    rec = Recorder()
    # a validation after every batch, windows of 3 micro-steps: the stop finds an open window of 2
    trainer = Trainer(max_epochs=MAX_EPOCHS, precision=16, limit_val_batches=1, val_check_interval=0.5,
                      accumulate_grad_batches=3, log_every_n_steps=1, callbacks=[ForcedMonitor(), es, rec])
    trainer.fit(module, dm)
    assert trainer.should_stop and trainer.early_stopping_callback is es
    assert (es.wait_count, es.best_score, es.stopped_epoch) == (1, 1.0, 0)
    assert len(trainer.val_history) == 2 and trainer.current_epoch == 0
    assert rec.hooks == ["fit_start", ("epoch_start", 0), ("validation_end", 0), ("validation_end", 0),
                         ("epoch_end", 0), "train_end"]
    # the open, partial accumulation window was discarded, not stepped
    assert trainer.global_step == 0 and trainer.runner.global_step == 0 and trainer.runner.micro_step == 0
    assert module.optimizer.step_count == 0


# ----------------------------------------------------------------------------------------------- main([...])
FH, FW = 64, 96


def _coco_clip(root):
    """2 videos of 3 JPEG frames of 64 x 96, categories 1 and 2 (as tests/test_gt_prompts_gpu.py builds its file)"""
    from PIL import Image

    from sam2_video.data import rle
    rng = np.random.default_rng(0)
    images, anns = [], []
    for v, video in enumerate(("a", "b")):
        for t in range(3):
            path = root / f"{video}_{t}.jpg"
            Image.fromarray(rng.integers(0, 256, (FH, FW, 3), dtype=np.uint8)).save(path, quality=95)
            image_id = 10 * v + t + 1
            images.append({"id": image_id, "video_id": video, "order_in_video": t, "height": FH, "width": FW,
                           "path": str(path), "file_name": path.name, "is_det_keyframe": not (v == 1 and t == 0)})
            for cat, (y, x) in ((1, (8 + 3 * t, 10 + 5 * v)), (2, (34, 50 + 4 * t))):
                m = np.zeros((FH, FW), bool)
                m[y:y + 18, x:x + 26] = True
                m[y + 6:y + 9, x + 8:x + 12] = False
                anns.append({"id": len(anns) + 1, "image_id": image_id, "category_id": cat,
                             "segmentation": rle.encode(m), "iscrowd": 0, "area": int(m.sum())})
    coco = {"images": images, "annotations": anns, "categories": [{"id": 1, "name": "one"}, {"id": 2, "name": "two"}]}
    path = root / "coco.json"
    path.write_text(json.dumps(coco))
    return str(path)


def test_main_runs_the_post_training_block(tmp_path, capsys):
    from sam2_video import train
    from sam2_video.eval import eval as E
    from sam2_video.training import callbacks as C
    data = tmp_path / "data"
    data.mkdir()
    coco_path = _coco_clip(data)
    run = tmp_path / "run"
    cfg = _sections()
    cfg["model"]["config_path"] = "tiny@256"  # the predictor of the post-training block, at the trained size
    cfg["trainer"].update(max_epochs=2, limit_train_batches=1, limit_val_batches=1, val_check_interval=1.0,
                          num_sanity_val_steps=0)
    cfg["callbacks"] = [{"_target_": "lightning.pytorch.callbacks.ModelCheckpoint", "monitor": "val/total_loss",
                         "mode": "min", "save_top_k": 1, "save_last": True, "dirpath": str(run / "checkpoints"),
                         "filename": REF_FILENAME},
                        {"_target_": "lightning.pytorch.callbacks.LearningRateMonitor", "logging_interval": "step"}]
    cfg["+callbacks"] = [{"_target_": "lightning.pytorch.callbacks.EarlyStopping", "monitor": "val/nope"}]  # dead key
    cfg["eval"].update(enabled=True, coco_path=coco_path, log_per_category=True)
    cfg_path = tmp_path / "cfg.json"
    cfg_path.write_text(json.dumps(cfg))
    np.random.seed(0)
    tr = train.main(["--config-json", str(cfg_path), "--run-dir", str(run)])
    ck = tr.checkpoint_callback
    assert type(ck) is C.ModelCheckpoint and len(tr.callbacks) == 2 and tr.early_stopping_callback is None
    assert tr.default_root_dir == str(run / "lightning_logs")
    assert os.path.isfile(ck.best_model_path) and os.path.isfile(run / "checkpoints" / "last.ckpt")
    for name in ("predict.json", "eval.pkl", "metrics.json", "prompt.pkl"):
        assert os.path.isfile(run / "eval" / name), name
    text = (run / "eval" / "metrics.json").read_text()
    metrics = json.loads(text)
    assert text == json.dumps(metrics, indent=2)
    want = E.eval(str(run / "eval" / "predict.json"), coco_path, str(tmp_path / "again"), score_on_device=False)
    assert metrics["eval/mIoU"] == float(want["avg_scores"]["iou"])
    assert metrics["eval/Dice"] == float(want["avg_scores"]["dice"])
    assert metrics["eval/MAE"] == float(want["avg_scores"]["mae"])
    assert all(np.isfinite(metrics[k]) for k in ("eval/mIoU", "eval/Dice", "eval/MAE"))
    assert metrics["best_checkpoint_path"] == ck.best_model_path
    for cat in (1, 2):
        for name, key in (("IoU", "iou"), ("Dice", "dice"), ("MAE", "mae")):
            assert metrics[f"eval/cat/{cat}/{name}"] == float(want["cat_scores"][cat][key])
    assert len(metrics) == 4 + 6
    assert len(json.loads((run / "eval" / "predict.json").read_text())) > 0
    # without an enabled eval section (or without the file) the block is skipped with one line on stderr
    capsys.readouterr()
    assert train.post_training_eval({"eval": {"enabled": True, "coco_path": str(tmp_path / "none.json")}}, tr,
                                    str(tmp_path / "skip")) is None
    assert train.post_training_eval({}, tr, str(tmp_path / "skip")) is None
    err = capsys.readouterr().err.strip().splitlines()
    assert len(err) == 2 and "none.json" in err[0] and "no eval section" in err[1]
    assert not os.path.exists(tmp_path / "skip")
