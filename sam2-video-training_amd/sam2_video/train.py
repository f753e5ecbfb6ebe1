"""Training entry point for the reference's config tree (reference train.py:30-127) when Hydra,
Lightning and W&B are not installed:

    python -m sam2_video.train --config-dir /path/to/configs --config-name best \\
        trainer.max_steps=100 data.train_path=... [+key=value ...]
    python -m sam2_video.train --config-json composed.json [key=value ...]   # an already composed tree
    python -m sam2_video.train ... --resume PATH | --resume last              # continue a killed run exactly

Composes the config (sam2_video.utils.config.compose: defaults list, interpolation,
overrides), seeds, instantiates `module` and `data_module` with `_recursive_=False`, the
`callbacks` list (train.py:110; absent = none; lightning.pytorch.callbacks.* resolve to
training/callbacks.py) and the `trainer` section with `callbacks=` and
`default_root_dir=<run_dir>/lightning_logs` (train.py:117-123; resolving
lightning.pytorch.trainer.trainer.Trainer to this build's Trainer), runs
`trainer.fit(module, data_module)` and writes a Lightning-layout checkpoint (`model.`-prefixed
state_dict) to <run_dir>/checkpoints/last.ckpt -- the final weights, the averaged ones after a
completed StochasticWeightAveraging run.  A literal `+callbacks` key (train.yaml) is the dead key
it is under Hydra.

Then the post-training block (train.py:135-231), when `eval.enabled` is set and `eval.coco_path`
exists: the best checkpoint (`trainer.checkpoint_callback.best_model_path`, `model.` prefix
stripped; none = the untuned weights, as the reference) -> `inference()` with the reference's
argument mapping (plus the optional `eval.num_correction_clicks` / `eval.correction_method`, this
build's corrective clicks before tracking) -> `eval()` -> <run_dir>/eval/metrics.json (eval/mIoU,
eval/Dice, eval/MAE, best_checkpoint_path; with `eval.log_per_category` also eval/cat/<id>/{IoU,Dice,MAE}, which the
reference sends to W&B only).  Unlike the reference, which raises, a missing `eval` section or an
enabled one whose COCO file does not exist prints one line to stderr and skips the block:
synthetic-data runs have no COCO file.  W&B logging and the baseline deltas
(extract_baseline_metrics) are not built.
"""
from __future__ import annotations

import argparse
import json
import os
import random
import sys

import torch


def main(argv=None, before_fit=None):
    """`before_fit(module, data_module, trainer)`, when given, runs right before trainer.fit (a test
    hook: e.g. the parity mode's dropout 0)"""
    ap = argparse.ArgumentParser()
    ap.add_argument("--config-dir", default="configs")
    ap.add_argument("--config-name", default="best")
    ap.add_argument("--config-json", default=None,
                    help="a config tree composed beforehand (JSON); overrides still apply")
    ap.add_argument("--run-dir", default=None)
    ap.add_argument("--resume", default=None, metavar="PATH",
                    help="continue the run this checkpoint was taken from (Trainer.fit(ckpt_path=PATH)); "
                         "'last' = <run_dir>/checkpoints/last.ckpt")
    ap.add_argument("overrides", nargs="*")
    args = ap.parse_args(argv)
    from .model.build import instantiate
    from .utils.config import apply_overrides, compose

    run_dir = args.run_dir or os.path.join("outputs", args.config_name)
    if args.config_json:
        with open(args.config_json) as f:
            cfg = apply_overrides(json.load(f), args.overrides)
    else:
        cfg = compose(args.config_dir, args.config_name, args.overrides, run_dir=run_dir)
    resume = args.resume
    if resume == "last":
        resume = os.path.join(run_dir, "checkpoints", "last.ckpt")
        if not os.path.isfile(resume):
            raise FileNotFoundError(f"--resume last: {resume} does not exist")
    seed = int(cfg.get("seed", 42))
    random.seed(seed)
    torch.manual_seed(seed)
    os.makedirs(run_dir, exist_ok=True)
    with open(os.path.join(run_dir, "config.json"), "w") as f:
        json.dump(cfg, f, indent=1, default=str)
    module = instantiate(cfg["module"], _recursive_=False)
    data_module = instantiate(cfg["data_module"], _recursive_=False)
    callbacks = [instantiate(cb) for cb in (cfg.get("callbacks") or [])]
    trainer = instantiate(cfg["trainer"], callbacks=callbacks,
                          default_root_dir=os.path.join(run_dir, "lightning_logs"))
    if before_fit is not None:
        before_fit(module, data_module, trainer)
    hist = trainer.fit(module, data_module, ckpt_path=resume)
    ck = os.path.join(run_dir, "checkpoints")
    os.makedirs(ck, exist_ok=True)
    trainer.save_checkpoint(os.path.join(ck, "last.ckpt"), module)
    for row in hist[-3:]:
        print(json.dumps(row), file=sys.stderr)
    post_training_eval(cfg, trainer, run_dir)
    return trainer


def post_training_eval(cfg, trainer, run_dir):
    """reference train.py:135-231 (module docstring) -> the metrics.json summary, or None when skipped"""
    ev = cfg.get("eval")
    if not isinstance(ev, dict):
        print("post-training eval skipped: the config has no eval section", file=sys.stderr)
        return None
    if not ev.get("enabled"):
        return None
    coco_path = ev.get("coco_path")
    if not coco_path or not os.path.exists(str(coco_path)):
        print(f"post-training eval skipped: eval.coco_path not found: {coco_path}", file=sys.stderr)
        return None
    import pickle

    from .eval import eval as eval_eval
    from .eval import inference as eval_infer
    cb = getattr(trainer, "checkpoint_callback", None)
    ckpt_path = cb.best_model_path if cb is not None else ""
    best_state_dict = None
    if ckpt_path:
        raw = torch.load(ckpt_path, map_location="cpu", weights_only=False)["state_dict"]
        if any(k.startswith("model.") for k in raw):
            best_state_dict = {k[len("model."):]: v for k, v in raw.items()}
        else:
            best_state_dict = raw
    model = cfg.get("model") or {}
    eval_infer.inference(
        run_dir=str(run_dir), coco_path=coco_path, output_path=ev.get("output_subdir"),
        prompt_type=ev.get("prompt_type"), clip_length=ev.get("clip_length"),
        variable_cats=ev.get("variable_cats", False), num_points=ev.get("num_points", 1),
        include_center=ev.get("include_center", True), noised_prompt=ev.get("noised_prompt", False),
        noise_intensity=ev.get("noise_intensity", 0.1), bbox_noise_type=ev.get("bbox_noise_type", "shift_scale"),
        num_neg_points=ev.get("num_neg_points", 0), grid_spaceing=ev.get("grid_spacing"),
        save_video_list=ev.get("save_video_list"), model_cfg_override=model.get("config_path"),
        sam2_checkpoint_override=model.get("checkpoint_path"), finetuned_state_dict=best_state_dict,
        num_correction_clicks=int(ev.get("num_correction_clicks", 0) or 0),
        correction_method=ev.get("correction_method", "center"))
    eval_dir = os.path.join(str(run_dir), "eval")
    os.makedirs(eval_dir, exist_ok=True)
    eval_eval.eval(predict_path=os.path.join(eval_dir, "predict.json"), coco_path=coco_path, output_path=eval_dir)
    with open(os.path.join(eval_dir, "eval.pkl"), "rb") as f:
        result = pickle.load(f)
    summary = {"eval/mIoU": float(result["avg_scores"]["iou"]), "eval/Dice": float(result["avg_scores"]["dice"]),
               "eval/MAE": float(result["avg_scores"]["mae"]), "best_checkpoint_path": ckpt_path}
    if ev.get("log_per_category"):
        for cat_id, scores in result["cat_scores"].items():
            for name, key in (("IoU", "iou"), ("Dice", "dice"), ("MAE", "mae")):
                summary[f"eval/cat/{cat_id}/{name}"] = float(scores[key])
    with open(os.path.join(eval_dir, "metrics.json"), "w") as f:
        json.dump(summary, f, indent=2)
    return summary


if __name__ == "__main__":
    main()
