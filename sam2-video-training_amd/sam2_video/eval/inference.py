"""The evaluation's inference surface -- sam2_video/eval/inference.py of the reference on the HIP predictor:
prompt a clip, propagate in reverse and then forward, write `predict.json` (one RLE per frame and category
with bbox and score) for the offline eval.py.

Restated under the reference's names with explicit arguments in place of its module globals (MOD, EVAL_DIR,
COCO_INFO, PROMPT_INFO, FINETUNED_STATE_DICT): add_prompt (inference.py:361-413), predict_on_video (:417-515),
process_video_clip (:532-577), save_as_coco_format (:845-915), _load_finetuned_weights_into_predictor
(:129-144).  No loguru, pycocotools or cv2: the RLE codec is data/rle.py.

What is new here is where the per-frame export runs.  The reference materialises [N, 1, H, W] fp32 logits per
tracked frame and issues, per object, a blocking `(logits[i] > 0).cpu().numpy()` and a blocking
`sigmoid(...).mean().item()`, then ORs bool images and RLE-encodes them on the host.  With
`export_on_device=True` (the default) predict_on_video drives SAM2VideoPredictor.propagate_in_video_export:
csrc/rle.hip thresholds, merges per category (`obj_id % mod`) and extracts the run boundaries from the
low-res logits, and only those, six integers per category and one float per object are copied, one frame
behind the tracking.  `export_on_device=False` is the reference's loop, kept as the A/B path and the tests'
oracle; save_as_coco_format writes the same file from either.

Threshold tuning runs on the same path: `sweep=` (a tune_threshold.SweepAccumulator) has csrc/rle.hip count,
per frame and category, the histogram of the merged logits over all candidate thresholds' logit cuts against the
ground truth -- a few hundred bytes in the frame's one copy instead of the reference's float16 probability dump
that tune_threshold.grid_search reloads per threshold -- and `threshold=` + save_thresholded_predict write
export_predict_from_probs.py's `predict_t0.xx.json` at the tuned threshold.  `probs_out_dir` and the two host
modules stay as the A/B path.

Out of scope: generating the prompts from ground truth (get_each_obj / generate_prompts_by_*: utils.py
mask_to_masks is cv2.morphologyEx + cv2.connectedComponentsWithStats, and cv2 is not a dependency -- a scipy
restatement could not be pinned against it) and the top-level `inference()` that drives it from a COCO file.
Callers build PromptInfo lists themselves (eval/utils.py) and call process_video_clip + save_as_coco_format.
"""
from __future__ import annotations

import json
import os
import pickle
from typing import Dict, List, Optional

import numpy as np
import torch

from ..data import rle
from .utils import ClipRange, PromptInfo, PromptObj, mask_to_bbox, sort_dicts_by_field

# train-time prompt names -> the names add_prompt switches on (inference.py:1004-1010)
PROMPT_TYPES = {"point": "points", "box": "bbox", "mask": "mask", "points": "points", "bbox": "bbox"}

_ABOVE_HALF = np.nextafter(np.float16(0.5), np.float16(1.0))  # 0.5 + 2^-11, the smallest float16 above one half


def _load_finetuned_weights_into_predictor(predictor, state_dict) -> None:
    """inference.py:129-144: a (mask decoder, prompt encoder or None) tuple is loaded strictly into the two
    modules, anything else through the predictor's load_state_dict(strict=False)"""
    if predictor is None:
        raise ValueError("predictor is None; cannot load fine-tuned weights")
    if state_dict is None:
        raise ValueError("state_dict is None; cannot load fine-tuned weights")
    if isinstance(state_dict, tuple):
        predictor.sam_mask_decoder.load_state_dict(state_dict[0], strict=True)
        if state_dict[1] is not None:
            predictor.sam_prompt_encoder.load_state_dict(state_dict[1], strict=True)
    else:
        predictor.load_state_dict(state_dict, strict=False)


def add_prompt(prompt_objs: List[PromptObj], predictor, inference_state, prompt_frame_order_in_video, prompt_type):
    """every object's prompt of one frame -> (predictor, inference_state, obj ids, video-res logits of the
    last call); prompt_type: points | bbox | mask (or the train-time point | box)"""
    prompt_type = PROMPT_TYPES.get(prompt_type, prompt_type)
    out_obj_ids, out_mask_logits = None, None
    for obj in prompt_objs:
        if prompt_type == "points":
            _, out_obj_ids, out_mask_logits = predictor.add_new_points_or_box(
                inference_state=inference_state, frame_idx=prompt_frame_order_in_video, obj_id=obj.obj_id,
                points=obj.points, labels=obj.pos_or_neg_label)
        elif prompt_type == "bbox":
            _, out_obj_ids, out_mask_logits = predictor.add_new_points_or_box(
                inference_state=inference_state, frame_idx=prompt_frame_order_in_video, obj_id=obj.obj_id,
                box=obj.bbox)
        elif prompt_type == "mask":
            _, out_obj_ids, out_mask_logits = predictor.add_new_mask(
                inference_state=inference_state, frame_idx=prompt_frame_order_in_video, obj_id=obj.obj_id,
                mask=torch.from_numpy(np.asarray(obj.mask)).to(torch.bool))
        else:
            raise ValueError(f"unknown prompt type {prompt_type!r} (points, bbox or mask)")
    return predictor, inference_state, out_obj_ids, out_mask_logits


def predict_on_video(predictor, inference_state, start_idx, frames=None, probs_out_dir: Optional[str] = None, *,
                     mod: Optional[int] = None, export_on_device: bool = True, threshold: Optional[float] = None,
                     sweep=None) -> Dict:
    """reverse pass, then forward pass (whose frames overwrite the reverse pass's: the prompt frame carries
    the forward result) -> {order_in_video: frame result}.

    export_on_device=False: the reference's structure, {obj_id: {"mask": bool [1, H, W] numpy, "score":
    float}} per frame, from propagate_in_video with two blocking copies per object.
    export_on_device=True: MergedFrame.result() per frame -- {"categories": {obj_id % mod: {"segmentation",
    "bbox", "area"}}, "scores": {obj_id: float}} -- with one frame in flight: frame t is waited for and
    string-encoded after frame t + 1 has been enqueued, so the copy and the host work overlap the tracking.

    probs_out_dir (with `frames`, the frame dicts of the video): one `<image id>.npz` per frame with the
    float16 sigmoid of the video-resolution logits and the metadata of inference.py:476-485; a tuning aid
    that materialises the logits for that frame in either mode.  One departure from the reference's bytes: a
    positive logit whose sigmoid rounds to exactly 0.5 in float16 (0 < v <= 2^-10) is stored as 0.5 + 2^-11,
    one float16 step up, so that `probs > 0.5` is `logits > 0`, the mask of predict.json, on every pixel.

    threshold (export_on_device only): the masks are binarised at that probability as the reference thresholds
    its float16 dump (export_predict_from_probs.py) and every frame result carries "max_logit" for
    save_thresholded_predict.  sweep (a tune_threshold.SweepAccumulator; export_on_device, `frames`): every
    tracked frame's histogram over the accumulator's cuts against its ground truth is counted on the device
    and added to it -- threshold tuning without a dump.  A frame both passes visit contributes once, from the
    first visit, as the dump's "skip if the file exists" keeps the reverse pass's probabilities."""
    if (threshold is not None or sweep is not None) and not export_on_device:
        raise ValueError("threshold= and sweep= run on the device export (export_on_device=True)")
    if sweep is not None and frames is None:
        raise ValueError("sweep= needs `frames` (the image id and size of every frame)")
    video_segments = {}
    frame_meta = None
    if frames is not None:
        frame_meta = {f["order_in_video"]: (f["id"], f["video_id"], int(f["height"]), int(f["width"])) for f in frames}

    def _maybe_write_probs(order_key, out_obj_ids, out_mask_logits):
        if probs_out_dir is None or frame_meta is None or len(out_obj_ids) == 0:
            return
        image_id, video_id, H, W = frame_meta[order_key]
        os.makedirs(probs_out_dir, exist_ok=True)
        npz_path = os.path.join(probs_out_dir, f"{image_id}.npz")
        if os.path.exists(npz_path):  # (so a frame both passes visit keeps the reverse pass's dump, as upstream)
            return
        logits = out_mask_logits.detach()
        probs = torch.sigmoid(logits).cpu().numpy().astype(np.float16)
        # float16 has no value between 0.5 and 0.5 + 2^-11: rounded to nearest, sigmoid(v) of 0 < v <= 2^-10 is
        # stored as exactly 0.5 and `probs > 0.5` loses pixels that `v > 0` -- the threshold of predict.json --
        # keeps.  Those pixels get the next float16 above one half, so the dump thresholds to the written masks.
        probs[(probs == np.float16(0.5)) & (logits > 0).cpu().numpy()] = _ABOVE_HALF
        probs = probs.reshape(len(out_obj_ids), probs.shape[-2], probs.shape[-1])
        np.savez_compressed(npz_path, probs=probs, obj_ids=np.asarray(out_obj_ids, dtype=np.int64),
                            image_id=np.int64(image_id), video_id=str(video_id),
                            order_in_video=np.int64(order_key), height=np.int32(H), width=np.int32(W))

    if not export_on_device:
        for reverse in (True, False):
            for out_frame_idx, out_obj_ids, out_mask_logits in predictor.propagate_in_video(inference_state,
                                                                                          reverse=reverse):
                order_key = out_frame_idx + start_idx
                _maybe_write_probs(order_key, out_obj_ids, out_mask_logits)
                video_segments[order_key] = {
                    out_obj_id: {"mask": (out_mask_logits[i] > 0.0).cpu().numpy(),
                                 "score": torch.sigmoid(out_mask_logits[i]).mean().item()}
                    for i, out_obj_id in enumerate(out_obj_ids)}
        return video_segments

    if mod is None:
        raise ValueError("predict_on_video(export_on_device=True) needs `mod` (category = obj_id % mod)")
    extra = {}
    if threshold is not None:
        extra["threshold"] = threshold
    if sweep is not None:
        # the ground truth of the whole clip, packed per category in the export's category order (first-seen
        # order of the objects), uploaded once
        if sweep.mod != mod:
            raise ValueError(f"the accumulator merges with mod {sweep.mod}, the export with {mod}")
        cat_ids = list(dict.fromkeys(i % mod for i in inference_state["obj_ids"]))
        gt = np.stack([sweep.gt_bits(frame_meta[t + start_idx][0], cat_ids, *frame_meta[t + start_idx][2:])
                       for t in range(inference_state["num_frames"])])
        gt = torch.from_numpy(gt).to(inference_state["device"])
        extra["sweep_cuts"], extra["gt_bits"] = sweep.cuts, lambda t: gt[t]

    def _collect(order_key, merged):
        video_segments[order_key] = res = merged.result()
        if sweep is not None and frame_meta[order_key][0] not in sweep:
            sweep.add_frame(frame_meta[order_key][0], merged.obj_ids, res["cat_ids"], res["sweep"])

    in_flight = None  # (order key, MergedFrame) of the frame enqueued last
    for reverse in (True, False):
        for out_frame_idx, out_obj_ids, merged in predictor.propagate_in_video_export(
                inference_state, lambda obj_id: obj_id % mod, reverse=reverse, **extra):
            order_key = out_frame_idx + start_idx
            if probs_out_dir is not None and frame_meta is not None:
                _maybe_write_probs(order_key, out_obj_ids,
                                   predictor._video_res(inference_state, merged.low_res_logits[:, None]))
            if in_flight is not None:
                _collect(*in_flight)
            in_flight = (order_key, merged)
    if in_flight is not None:
        _collect(*in_flight)
    return video_segments


def _read_frames(paths) -> np.ndarray:
    """image files -> [T, H, W, 3] uint8 (what the reference reaches through a folder of symlinks)"""
    from PIL import Image
    return np.stack([np.asarray(Image.open(p).convert("RGB")) for p in paths])


def process_video_clip(predictor, frames, clip_prompts: List[PromptInfo], clip_range: ClipRange,
                       probs_out_dir: Optional[str] = None, *, video=None, mod: Optional[int] = None,
                       export_on_device: bool = True, finetuned_state_dict=None, threshold: Optional[float] = None,
                       sweep=None) -> Dict:
    """inference.py:532-577 on a predictor the caller built: init_state on the clip's frames, the clip's
    prompts, predict_on_video.  `frames`: the video's frame dicts (id, video_id, order_in_video, height,
    width, path), indexed by order_in_video as in the reference.  `video`: the clip's images as a list of
    paths, a JPEG folder or a [T, H, W, 3] uint8 array; default: the `path` of frames[start_idx:end_idx + 1]."""
    start_idx, end_idx = clip_range.start_idx, clip_range.end_idx
    if video is None:
        video = [f["path"] for f in frames[start_idx:end_idx + 1]]
    if isinstance(video, (list, tuple)) and video and isinstance(video[0], (str, os.PathLike)):
        video = _read_frames(video)
    if finetuned_state_dict is not None:
        _load_finetuned_weights_into_predictor(predictor, finetuned_state_dict)
    inference_state = predictor.init_state(video_path=video)
    for prompt_info in clip_prompts:
        add_prompt(prompt_info.prompt_objs, predictor, inference_state, prompt_info.frame_idx - start_idx,
                   prompt_info.prompt_type)
    return predict_on_video(predictor, inference_state, start_idx, frames=frames, probs_out_dir=probs_out_dir,
                            mod=mod, export_on_device=export_on_device, threshold=threshold, sweep=sweep)


def _frame_annotations(image_id, segment, mod) -> List[Dict]:
    """the annotations of one frame from either structure of predict_on_video"""
    if "categories" in segment:  # MergedFrame.result(): merged, encoded and measured on the device
        score = None
        for score in segment["scores"].values():
            pass  # (the last object's score: see below)
        return [{"image_id": image_id, "category_id": cat, "segmentation": dict(info["segmentation"]),
                 "bbox": list(info["bbox"]), "iscrowd": 0, "score": score}
                for cat, info in segment["categories"].items()]
    merged_mask = {}
    score = None
    for key, mask_info in segment.items():
        remainder = key % mod
        m_mask = np.logical_or.reduce(mask_info["mask"], axis=0)
        # The reference assigns `score` here, inside the merge loop, and reads it in the loop below
        # (inference.py:873-899): every annotation of a frame carries the score of the LAST object of the
        # frame's dict, whatever its category.  Kept, because a drop-in writes the same file.
        score = mask_info["score"]
        merged_mask[remainder] = m_mask if remainder not in merged_mask else np.logical_or(merged_mask[remainder],
                                                                                          m_mask)
    out = []
    for key, mask in merged_mask.items():
        if mask.sum() == 0:
            continue
        out.append({"image_id": image_id, "category_id": key, "segmentation": rle.encode(mask),
                    "bbox": mask_to_bbox(mask), "iscrowd": 0, "score": score})
    return out


def save_as_coco_format(all_video_segments, frames_by_video, mod, eval_dir, prompt_info=None, save_video_list=None):
    """inference.py:845-915: {video_id: predict_on_video's result} -> `<eval_dir>/predict.json` (indent=4;
    per annotation image_id, category_id, segmentation, bbox, iscrowd 0, score) and `<eval_dir>/prompt.pkl`.
    frames_by_video: {video_id: the video's frame dicts}; frames are written in order_in_video, categories in
    first-seen order of the frame's objects, empty merged masks are skipped.  -> (predict path, prompt path)"""
    if save_video_list is None:
        save_video_list = list(all_video_segments)
    coco_annotations: List[Dict] = []
    for video_id in save_video_list:
        video_segments = all_video_segments[video_id]
        for frame in sort_dicts_by_field(frames_by_video[video_id], "order_in_video"):
            coco_annotations.extend(_frame_annotations(frame["id"], video_segments[frame["order_in_video"]], mod))
    os.makedirs(eval_dir, exist_ok=True)
    predict_path = os.path.join(eval_dir, "predict.json")
    prompt_path = os.path.join(eval_dir, "prompt.pkl")
    with open(predict_path, "w") as f:
        json.dump(coco_annotations, f, indent=4)
    with open(prompt_path, "wb") as f:
        pickle.dump(list(prompt_info or []), f)
    return predict_path, prompt_path


def save_thresholded_predict(all_video_segments, frames_by_video, threshold, output_predict: Optional[str] = None,
                             exclude_background: bool = False) -> str:
    """what export_predict_from_probs.export_predict writes from a dump, from predict_on_video(threshold=...)'s
    device results: per frame and non-empty category image_id, category_id, segmentation, bbox, iscrowd 0 and
    score = the category's maximum float16 probability, float16(sigmoid(max over its objects of max_logit)).
    indent=2; default name `predict_t{threshold:.2f}.json` (in the working directory).  -> the path"""
    annotations: List[Dict] = []
    for video_id, video_segments in all_video_segments.items():
        for frame in sort_dicts_by_field(frames_by_video[video_id], "order_in_video"):
            segment = video_segments[frame["order_in_video"]]
            if "max_logit" not in segment:
                raise ValueError("save_thresholded_predict needs the results of predict_on_video(threshold=...)")
            for cat, info in segment["categories"].items():
                if exclude_background and cat == 0:
                    continue
                m = max(float(v) for i, v in segment["max_logit"].items() if segment["obj_cats"][i] == cat)
                score = float(np.float16(1.0 / (1.0 + np.exp(-np.float64(m)))))
                annotations.append({"image_id": int(frame["id"]), "category_id": int(cat),
                                    "segmentation": dict(info["segmentation"]), "bbox": list(info["bbox"]),
                                    "iscrowd": 0, "score": score})
    if output_predict is None:
        output_predict = f"predict_t{threshold:.2f}.json"
    with open(output_predict, "w") as f:
        json.dump(annotations, f, indent=2)
    return output_predict
