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

Prompts from ground truth and the driver: get_each_obj (:275-326), find_prompt_frame (:147-175),
generate_prompts_by_clip_length / _by_categories (:598-703), merge_prompts (:706-767), process_singel_video,
process_all_videos (:771-841) and inference() (:919-1085) over a CocoIndex (no pycocotools).  With
`on_device=True` get_each_obj runs a prompt frame's annotations as one batch through csrc/gtprompt.hip and
csrc/cc.hip -- RLE decode, the 10 x 10 closing, labelling, the kept components with their boxes and centre sums,
and the pixel of every drawn rank -- with two copies to the host; the random draws are the reference's
np.random.choice calls in the reference's order, so both paths give the same prompts under the same seed.
`on_device=False` is eval/utils.py mask_to_masks / mask_to_points, the A/B path.  The closing's window is
eval/utils.py CLOSE_DILATE_WINDOW: it follows OpenCV's documented formulas, and the masks the reference's own
cv2 opening wrote agree with it ("Dataset preparation on the device").

Correction clicks (upstream's interactive protocol: prompt, then N corrective clicks, then track):
add_correction_clicks compares the prompt frame's video-resolution logits with the objects' ground-truth masks
and feeds the next click of every object back through add_new_points_or_box(clear_old_points=False), for
`num_correction_clicks` rounds.  The clicks come from model/modeling/sam2_utils.py get_next_point -- on
csrc/clicks.hip with `clicks_on_device=True`: one batched call and one copy of B clicks per round, where the
reference's samplers copy two full-resolution masks per object to the host.  Off (0 clicks) by default.

Out of scope: PromptObjNoiseAdder (`noised_prompt=True` raises: it needs albumentations) and the reference's
dead helpers generate_negative_samples, fluctuate_point and get_obj_from_masks.
"""
from __future__ import annotations

import json
import os
import pickle
from dataclasses import dataclass
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from ..data import rle
from . import utils as _utils
from .utils import ClipRange, PromptInfo, PromptObj, mask_to_bbox, sort_dicts_by_field

# what inference() builds when no predictor is passed (the reference's module globals model_cfg / sam2_checkpoint;
# its checkpoint path is site-specific, so the default here is the builder's own)
MODEL_CFG = "sam2_hiera_t.yaml"
SAM2_CHECKPOINT = None

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


def add_correction_clicks(prompt_objs: List[PromptObj], predictor, inference_state, frame_idx, out_mask_logits,
                          n_clicks, method="center", on_device=True):
    """n_clicks rounds of corrective clicks on one prompted frame: per round the frame's video-resolution logits
    of all objects (out_mask_logits [N, 1, H, W], what add_prompt or the round before returned) are thresholded
    at 0 and compared with the objects' ground truth (PromptObj.mask, uploaded once), get_next_point gives one
    click per object in one batched call, the B clicks come to the host in one copy, and every object is refined
    with add_new_points_or_box(clear_old_points=False).  The clicks are appended to each PromptObj's points /
    pos_or_neg_label (so prompt.pkl records them).  method: "center" (the centre of the larger error region) or
    "uniform" (a uniformly drawn error pixel; its generator is seeded from np.random.randint, so np.random.seed
    fixes the run like the prompt draws).  on_device=False: the samplers' host twin.  -> the last logits"""
    from ..model.modeling.sam2_utils import get_next_point
    if method not in ("center", "uniform"):
        raise ValueError(f"unknown sampling method {method}")
    if n_clicks <= 0 or not prompt_objs:
        return out_mask_logits
    device = out_mask_logits.device
    rows = [inference_state["obj_ids"].index(obj.obj_id) for obj in prompt_objs]
    gt = torch.from_numpy(np.stack([np.asarray(obj.mask, dtype=bool) for obj in prompt_objs])[:, None]).to(device)
    if gt.shape[-2:] != out_mask_logits.shape[-2:]:
        raise ValueError(f"the ground-truth masks are {tuple(gt.shape[-2:])}, the video is "
                         f"{tuple(out_mask_logits.shape[-2:])}")
    generator = None
    if method == "uniform":
        generator = torch.Generator(device=device)
        generator.manual_seed(int(np.random.randint(0, 2 ** 31 - 1)))
    rows_d = torch.as_tensor(rows, device=device)
    for _ in range(int(n_clicks)):
        pred = out_mask_logits.index_select(0, rows_d) > 0
        points, labels = get_next_point(gt, pred, method, generator=generator, on_device=on_device)
        clicks = torch.cat([points.reshape(len(rows), 2), labels.reshape(len(rows), 1).to(torch.float32)],
                           dim=1).cpu().numpy()  # the round's B clicks in one copy
        for obj, (x, y, label) in zip(prompt_objs, clicks):
            _, _, out_mask_logits = predictor.add_new_points_or_box(
                inference_state=inference_state, frame_idx=frame_idx, obj_id=obj.obj_id,
                points=np.array([[x, y]], dtype=np.float32), labels=np.array([label], dtype=np.int32),
                clear_old_points=False)
            pts = np.asarray(obj.points)
            obj.points = np.concatenate([pts.reshape(-1, 2), np.array([[x, y]]).astype(pts.dtype)], axis=0)
            lab = np.asarray(obj.pos_or_neg_label)
            obj.pos_or_neg_label = np.concatenate([lab, np.array([label]).astype(lab.dtype)])
    return out_mask_logits


def _check_clicks(prompt_type, num_correction_clicks):
    if num_correction_clicks and PROMPT_TYPES.get(prompt_type, prompt_type) == "mask":
        raise ValueError("correction clicks with the mask prompt type: the prompt already is the ground truth")
    if num_correction_clicks < 0:
        raise ValueError(f"num_correction_clicks is {num_correction_clicks}")


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
                       sweep=None, num_correction_clicks: int = 0, correction_method: str = "center",
                       clicks_on_device: bool = True) -> Dict:
    """inference.py:532-577 on a predictor the caller built: init_state on the clip's frames, the clip's
    prompts, predict_on_video.  `frames`: the video's frame dicts (id, video_id, order_in_video, height,
    width, path), indexed by order_in_video as in the reference.  `video`: the clip's images as a list of
    paths, a JPEG folder or a [T, H, W, 3] uint8 array; default: the `path` of frames[start_idx:end_idx + 1].
    num_correction_clicks > 0: every prompt frame's objects get that many corrective clicks before tracking
    (add_correction_clicks; correction_method center | uniform, clicks_on_device False = the host twin)."""
    for prompt_info in clip_prompts:
        _check_clicks(prompt_info.prompt_type, num_correction_clicks)
    start_idx, end_idx = clip_range.start_idx, clip_range.end_idx
    if video is None:
        video = [f["path"] for f in frames[start_idx:end_idx + 1]]
    if isinstance(video, (list, tuple)) and video and isinstance(video[0], (str, os.PathLike)):
        video = _read_frames(video)
    if finetuned_state_dict is not None:
        _load_finetuned_weights_into_predictor(predictor, finetuned_state_dict)
    inference_state = predictor.init_state(video_path=video)
    for prompt_info in clip_prompts:
        _, _, _, logits = add_prompt(prompt_info.prompt_objs, predictor, inference_state,
                                     prompt_info.frame_idx - start_idx, prompt_info.prompt_type)
        if num_correction_clicks:
            add_correction_clicks(prompt_info.prompt_objs, predictor, inference_state,
                                  prompt_info.frame_idx - start_idx, logits, num_correction_clicks,
                                  method=correction_method, on_device=clicks_on_device)
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


# ------------------------------------------------------------------------------ prompts from ground truth
class CocoIndex:
    """what the driver reads of a COCO file (the pycocotools.COCO calls of the reference): the images, the
    annotations of an image and the category ids, all in file order; mod = max(category ids) + 1"""

    def __init__(self, coco):
        if not isinstance(coco, dict):
            with open(coco, "r") as f:
                coco = json.load(f)
        self.dataset = coco
        self.imgs: List[Dict] = list(coco.get("images", []))
        self.cat_ids: List[int] = [c["id"] for c in coco.get("categories", [])]
        self.anns_by_image: Dict = {}
        for a in coco.get("annotations", []):
            self.anns_by_image.setdefault(a["image_id"], []).append(a)
        self.mod = max(self.cat_ids) + 1

    def anns(self, image_id) -> List[Dict]:
        return self.anns_by_image.get(image_id, [])

    def video_ids(self) -> List:
        """first-seen order (the reference iterates a set)"""
        return list(dict.fromkeys(img["video_id"] for img in self.imgs))

    def frames(self, video_id) -> List[Dict]:
        return _utils.get_dicts_by_field_value(self.imgs, "video_id", video_id)


def _draw_ranks(n: int, num_points: int, include_center: bool):
    """the draws mask_to_points makes on a mask with n (grid-selected) pixels, without the pixels: -> (whether the
    centre leads the result, the ranks of the sampled pixels in np.argwhere order).  The same early return and
    the same np.random.choice call on the global generator as eval/utils.py mask_to_points."""
    if include_center is True:
        num_points -= 1
    if num_points > n:
        return False, np.arange(n, dtype=np.int64)
    return bool(include_center), np.random.choice(n, num_points, replace=False)


def _host_objs(anns, mod, obj_count, num_points, num_neg_points, include_center):
    objs = []
    for ann in anns:
        for mask in _utils.mask_to_masks(rle.decode(ann["segmentation"])):
            pos = _utils.mask_to_points(mask, num_points=num_points, include_center=include_center)
            neg = _utils.mask_to_points(np.logical_not(mask), num_points=num_neg_points, include_center=False)
            objs.append(PromptObj(mask=mask, bbox=mask_to_bbox(mask), points=np.concatenate([pos, neg]),
                                  obj_id=obj_count * mod + ann["category_id"],
                                  pos_or_neg_label=np.concatenate([np.ones(len(pos)), np.zeros(len(neg))])))
            obj_count += 1
    return objs, obj_count


def _device_objs(anns, mod, obj_count, num_points, num_neg_points, include_center, device):
    from ..kernels import ops
    counts, size = [], None
    for ann in anns:
        seg = rle._as_rle(ann["segmentation"])
        hw = [int(v) for v in seg["size"]]
        if size is not None and hw != size:
            raise ValueError(f"annotations of image {ann.get('image_id')} have sizes {size} and {hw}")
        size = hw
        c = seg["counts"]
        if isinstance(c, bytes):
            c = c.decode("ascii")
        counts.append(rle.counts_from_string(c) if isinstance(c, str) else list(c))
    if not anns:
        return [], obj_count
    H, W = size
    A = len(anns)
    grid_host = _utils.GRID
    grid = None
    if grid_host is not None:
        if grid_host.shape != (H, W):
            raise ValueError(f"GRID is {grid_host.shape}, the frame's masks are {(H, W)}")
        grid = torch.from_numpy(np.ascontiguousarray(grid_host, dtype=np.uint8)).to(device)
    yw, ew = _utils.CLOSE_DILATE_WINDOW, _utils.CLOSE_ERODE_WINDOW
    raw = ops.rle_decode(counts, H, W, device=device)
    closed = ops.morph_rect(ops.morph_rect(raw, "dilate", yw, yw), "erode", ew, ew)
    labels, areas = ops.cc_label_u8(closed)
    hdr_d, stats_d, index_d = ops.cc_components(labels, areas, _utils.MIN_COMPONENT_AREA, grid=grid)
    # header, stats and index image in one copy
    packed = torch.cat([hdr_d.view(torch.uint8), stats_d.reshape(-1).view(torch.uint8), index_d.reshape(-1)]).cpu().numpy()
    nh, ns = hdr_d.numel() * 4, stats_d.numel() * 8
    hdr = packed[:nh].view(np.int32)
    stats = packed[nh:nh + ns].view(np.int64).reshape(-1, ops.GP_STATS)
    index = packed[nh + ns:].reshape(A, H, W)
    if hdr[2 * A + 1] != 0:
        raise RuntimeError(f"an annotation closes into more than {ops.GP_MAX_INDEX} components of area >= "
                           f"{_utils.MIN_COMPONENT_AREA}: the uint8 index image cannot name them")
    n_domain = int(grid_host.sum()) if grid_host is not None else H * W
    # the host draws, in the reference's order: per component the positives, then the negatives
    plan, queries = [], []
    for a, ann in enumerate(anns):
        cnt, off = int(hdr[2 * a]), int(hdr[2 * a + 1])
        for j in range(cnt):
            label, area, xmin, ymin, xmax, ymax, n_sel, sx, sy = (int(v) for v in stats[off + j])
            use_center, pos_ranks = _draw_ranks(n_sel, num_points, include_center)
            _, neg_ranks = _draw_ranks(n_domain - n_sel, num_neg_points, False)
            center = None
            if use_center:
                # Sum // n equals the reference's float64 mean truncated: the sums are exact in float64
                # (< 2^53), and a quotient just below an integer k <= 2^24 is at least 1 / n >= 2^-24 below it,
                # far more than float64's spacing there, so the division cannot round up to k.
                center = (np.array([[sx // n_sel, sy // n_sel]], dtype=np.int64) if n_sel > 0 else
                          np.mean(np.zeros((0, 2), dtype=np.int64), axis=0).astype(int).reshape(1, -1))
            q0 = len(queries)
            queries += [(a, label, 0, int(r), n_sel) for r in pos_ranks]
            queries += [(a, label, 1, int(r), n_domain - n_sel) for r in neg_ranks]
            plan.append((a, j, ann["category_id"], [xmin, ymin, xmax, ymax], center, q0, len(pos_ranks), len(neg_ranks)))
    if queries:
        q = torch.from_numpy(np.asarray([t[:4] for t in queries], dtype=np.int32).T.copy()).to(device)
        xy_d, count_d = ops.mask_rank_select(q[0], q[1], q[2], q[3], labels, grid=grid)
        out = torch.cat([xy_d.reshape(-1), count_d]).cpu().numpy()  # the points in one copy
        xy, count = out[:2 * len(queries)].reshape(-1, 2).astype(np.int64), out[2 * len(queries):]
        want = np.asarray([t[4] for t in queries])
        if not np.array_equal(count, want) or (xy < 0).any():
            raise RuntimeError("s2h_mask_rank_select disagrees with s2h_cc_components about the pixel counts")
    else:
        xy = np.zeros((0, 2), dtype=np.int64)
    objs = []
    for a, j, cat, box, center, q0, n_pos, n_neg in plan:
        pos = xy[q0:q0 + n_pos]
        if center is not None:
            pos = np.concatenate([center, pos], axis=0)
        neg = xy[q0 + n_pos:q0 + n_pos + n_neg]
        objs.append(PromptObj(mask=index[a] == j + 1, bbox=[float(v) for v in box], points=np.concatenate([pos, neg]),
                              obj_id=obj_count * mod + cat,
                              pos_or_neg_label=np.concatenate([np.ones(len(pos)), np.zeros(len(neg))])))
        obj_count += 1
    return objs, obj_count


def get_each_obj(coco: CocoIndex, prompt_frame, *, mod, obj_count, num_points, num_neg_points, include_center,
                 cats=None, on_device: bool = True, device="cuda") -> Tuple[List[PromptObj], int]:
    """inference.py:275-326 with its globals as arguments: every annotation of the frame (of the categories
    `cats` when given) is closed and split into its components of area >= 10 (mask_to_masks), and every
    component becomes a PromptObj -- mask (host bool [H, W] of the closed component), bbox [xmin, ymin, xmax,
    ymax] floats, points int64 [k, 2] (x, y): the positives (centre first when include_center) then the
    negatives, pos_or_neg_label float64 ones then zeros, obj_id = obj_count * mod + category_id with obj_count
    incremented per component.  -> (objs, the new obj_count).

    on_device: the frame's annotations as one batch through the HIP kernels (module docstring), two copies to the
    host; the random stream is the reference's: per component np.random.choice(n_sel, k, replace=False) for the
    positives, then np.random.choice(n_neg, num_neg_points, replace=False) for the negatives, on the global numpy
    generator, with mask_to_points' early returns -- so both paths return equal objects under one seed."""
    anns = [a for a in coco.anns(prompt_frame["id"]) if cats is None or a["category_id"] in cats]
    if on_device:
        return _device_objs(anns, mod, obj_count, num_points, num_neg_points, include_center, device)
    return _host_objs(anns, mod, obj_count, num_points, num_neg_points, include_center)


@dataclass
class PromptGen:
    """the reference's prompt globals (COCO_INFO, MOD, OBJ_COUNT, NUM_POINTS, NUM_NEG_POINTS, INCLUDE_CENTER) for
    one run: objs(frame) is get_each_obj(frame) with the running object count"""

    coco: CocoIndex
    num_points: int = 1
    num_neg_points: int = 0
    include_center: bool = True
    on_device: bool = True
    device: str = "cuda"
    obj_count: int = 0

    def objs(self, frame, cats=None) -> List[PromptObj]:
        objs, self.obj_count = get_each_obj(self.coco, frame, mod=self.coco.mod, obj_count=self.obj_count,
                                            num_points=self.num_points, num_neg_points=self.num_neg_points,
                                            include_center=self.include_center, cats=cats, on_device=self.on_device,
                                            device=self.device)
        return objs


def find_prompt_frame(coco: CocoIndex, frames, clip_range: ClipRange):
    """the first keyframe (is_det_keyframe is not False) inside the clip that has annotations, or None"""
    for frame in frames:
        if frame.get("is_det_keyframe") is False:
            continue
        if frame["order_in_video"] < clip_range.start_idx or frame["order_in_video"] > clip_range.end_idx:
            continue
        if not coco.anns(frame["id"]):
            continue
        return frame
    return None


def _prompt_info(gen: PromptGen, frame, prompt_type) -> PromptInfo:
    return PromptInfo(prompt_objs=gen.objs(frame), frame_idx=frame["order_in_video"], prompt_type=prompt_type,
                      video_id=str(frame["video_id"]), path=frame["path"], clip_range=None)


def generate_prompts_by_categories(gen: PromptGen, frames, prompt_type: str):
    """inference.py:598-654: a new clip starts at every keyframe that shows a category not seen before;
    yields ([PromptInfo], ClipRange)"""
    existing, prev, prev_start, out = set(), None, None, []
    for frame in frames:
        if frame.get("is_det_keyframe") is False:
            continue
        frame_cats = {a["category_id"] for a in gen.coco.anns(frame["id"])}
        if frame_cats.issubset(existing):
            continue
        existing |= frame_cats
        info = _prompt_info(gen, frame, prompt_type)
        if prev is not None:
            prev.clip_range = ClipRange(prev_start, info.frame_idx - 1)
            out.append(([prev], ClipRange(prev_start, info.frame_idx - 1)))
        prev, prev_start = info, info.frame_idx
    if prev is not None and prev_start != len(frames) - 1:  # (as the reference: a last clip of one frame is dropped)
        prev.clip_range = ClipRange(prev_start, len(frames) - 1)
        out.append(([prev], ClipRange(prev_start, len(frames) - 1)))
    yield from out


def generate_prompts_by_clip_length(gen: PromptGen, frames, prompt_type, clip_length: Optional[int]):
    """inference.py:657-703: clips of clip_length frames (None: the whole video), each prompted on its first
    annotated keyframe; a range without one is absorbed into the clip before it; yields ([PromptInfo], ClipRange)"""
    if clip_length is None:
        clip_length = len(frames)
    cur_start, cur_end, cur_prompts = 0, -1, []
    for start_idx in range(0, len(frames), clip_length):
        end_idx = min(start_idx + clip_length - 1, len(frames) - 1)
        prompt_frame = find_prompt_frame(gen.coco, frames, ClipRange(start_idx, end_idx))
        if prompt_frame is None:
            cur_end = end_idx
            continue
        if cur_start <= cur_end:
            for p in cur_prompts:
                p.clip_range = ClipRange(cur_start, cur_end)
            yield cur_prompts, ClipRange(cur_start, cur_end)
            cur_prompts = []
        cur_prompts.append(_prompt_info(gen, prompt_frame, prompt_type))
        cur_start, cur_end = start_idx, end_idx
    if cur_start <= cur_end:
        for p in cur_prompts:
            p.clip_range = ClipRange(cur_start, cur_end)
        yield cur_prompts, ClipRange(cur_start, cur_end)


def merge_prompts(prompts_by_categories: Iterable, prompts_by_clip_length: Iterable):
    """inference.py:706-767: the two range lists keyed by start index (a clip-length range replaces a category
    range with the same start), sorted; a range that starts before the running one ends cuts it short"""
    ranges = {}
    for prompts, clip_range in list(prompts_by_categories) + list(prompts_by_clip_length):
        ranges[clip_range.start_idx] = (prompts, clip_range)
    merged, cur = [], None  # cur: [start, end, prompts]
    for prompts, clip_range in sorted(ranges.values(), key=lambda x: x[1].start_idx):
        if cur is not None:
            end = clip_range.start_idx - 1 if clip_range.start_idx < cur[1] else cur[1]
            for p in cur[2]:
                p.clip_range = ClipRange(cur[0], end)
            merged.append((cur[2], ClipRange(cur[0], end)))
        cur = [clip_range.start_idx, clip_range.end_idx, prompts]
    if cur is not None:
        for p in cur[2]:
            p.clip_range = ClipRange(cur[0], cur[1])
        merged.append((cur[2], ClipRange(cur[0], cur[1])))
    return merged


def process_singel_video(predictor, gen: PromptGen, frames, prompt_type, clip_length: Optional[int] = None,
                         variable_cats: bool = False, probs_out_dir=None, *, prompt_log: Optional[List] = None,
                         export_on_device: bool = True, threshold: Optional[float] = None, sweep=None,
                         num_correction_clicks: int = 0, correction_method: str = "center",
                         clicks_on_device: bool = True) -> Dict:
    """inference.py:771-814 (the reference's spelling): the object count restarts, the video's clips are prompted
    and tracked one after the other on `predictor`; every clip's PromptInfo list is appended to prompt_log"""
    gen.obj_count = 0
    if variable_cats:
        clips = merge_prompts(generate_prompts_by_categories(gen, frames, prompt_type),
                              generate_prompts_by_clip_length(gen, frames, prompt_type, clip_length))
    else:
        clips = generate_prompts_by_clip_length(gen, frames, prompt_type, clip_length)
    video_segments = {}
    for clip_prompts, clip_range in clips:
        if prompt_log is not None:
            prompt_log.extend(clip_prompts)
        video_segments.update(process_video_clip(predictor, frames, clip_prompts, clip_range,
                                                 probs_out_dir=probs_out_dir, mod=gen.coco.mod,
                                                 export_on_device=export_on_device, threshold=threshold, sweep=sweep,
                                                 num_correction_clicks=num_correction_clicks,
                                                 correction_method=correction_method,
                                                 clicks_on_device=clicks_on_device))
    return video_segments


def process_all_videos(predictor, gen: PromptGen, prompt_type, clip_length, variable_cats, probs_out_dir=None, *,
                       prompt_log: Optional[List] = None, export_on_device: bool = True,
                       threshold: Optional[float] = None, sweep=None, num_correction_clicks: int = 0,
                       correction_method: str = "center", clicks_on_device: bool = True) -> Dict:
    """inference.py:818-841: {video_id: process_singel_video's result}, the videos in first-seen order"""
    return {video_id: process_singel_video(predictor, gen, gen.coco.frames(video_id), prompt_type, clip_length,
                                           variable_cats, probs_out_dir=probs_out_dir, prompt_log=prompt_log,
                                           export_on_device=export_on_device, threshold=threshold, sweep=sweep,
                                           num_correction_clicks=num_correction_clicks,
                                           correction_method=correction_method, clicks_on_device=clicks_on_device)
            for video_id in gen.coco.video_ids()}


def inference(coco_path, output_path, prompt_type, save_video_list=None, clip_length=None, variable_cats=False,
              num_points=1, include_center=True, noised_prompt=False, noise_intensity=0.1,
              bbox_noise_type="shift_scale", num_neg_points=0, grid_spaceing=None, probs_out_dir: Optional[str] = None,
              *, run_dir, model_cfg_override: Optional[str] = None, sam2_checkpoint_override: Optional[str] = None,
              finetuned_state_dict=None, predictor=None, prompts_on_device: bool = True,
              export_on_device: bool = True, threshold: Optional[float] = None, sweep=None,
              num_correction_clicks: int = 0, correction_method: str = "center", clicks_on_device: bool = True):
    """inference.py:919-1085: prompts from the ground truth of `coco_path` (a COCO file whose images carry
    video_id, order_in_video, is_det_keyframe, path, height and width), every video tracked clip by clip,
    `<run_dir>/eval/predict.json` and `prompt.pkl` written -> (predict path, prompt path).  prompt_type: point |
    box | mask (or points | bbox); clip_length None = one clip per video; variable_cats: a new clip also starts
    where a new category appears; grid_spaceing: sample the points on a grid (init_grid on the first image's
    size; like the reference, None leaves an earlier grid in place); probs_out_dir (relative: under the eval
    directory): the float16 probability dumps and their meta.json.  `output_path` is unused, as in the reference.

    Beyond the reference: predictor (None: built once with build_sam2_video_predictor from model_cfg_override /
    sam2_checkpoint_override or the module's MODEL_CFG / SAM2_CHECKPOINT, and reused for every clip);
    prompts_on_device (get_each_obj on the HIP kernels); export_on_device, threshold, sweep: see predict_on_video;
    num_correction_clicks (0: none), correction_method (center | uniform), clicks_on_device: every prompt frame's
    objects get that many corrective clicks against their ground truth before the clip is tracked
    (add_correction_clicks); with the mask prompt type a nonzero count raises ValueError.

    Differences from the reference: the predictor is built (and finetuned_state_dict loaded) once, not per clip;
    the videos are processed in first-seen order (the reference iterates a set); prompt.pkl holds this call's
    PromptInfo list only (the reference's module global accumulates across calls); noised_prompt=True raises
    NotImplementedError (PromptObjNoiseAdder needs albumentations and is not restated), so noise_intensity and
    bbox_noise_type are unused; the dead helpers generate_negative_samples, fluctuate_point and
    get_obj_from_masks are not restated."""
    if noised_prompt:
        raise NotImplementedError("noised_prompt=True needs PromptObjNoiseAdder, which is built on albumentations "
                                  "and is not part of this package")
    if run_dir is None or str(run_dir).strip() == "":
        raise ValueError("inference(): run_dir must be provided and non-empty")
    _check_clicks(prompt_type, num_correction_clicks)
    if correction_method not in ("center", "uniform"):
        raise ValueError(f"unknown sampling method {correction_method}")
    eval_dir = os.path.join(str(run_dir), "eval")
    os.makedirs(eval_dir, exist_ok=True)
    coco = CocoIndex(coco_path)
    if grid_spaceing is not None:
        _utils.init_grid((coco.imgs[0]["height"], coco.imgs[0]["width"]), grid_spaceing)
    if probs_out_dir is not None:
        if not os.path.isabs(probs_out_dir):
            probs_out_dir = os.path.join(eval_dir, probs_out_dir)
        os.makedirs(probs_out_dir, exist_ok=True)
    if predictor is None:
        from ..predictor import build_sam2_video_predictor
        predictor = build_sam2_video_predictor(model_cfg_override or MODEL_CFG,
                                               sam2_checkpoint_override or SAM2_CHECKPOINT)
    if finetuned_state_dict is not None:
        _load_finetuned_weights_into_predictor(predictor, finetuned_state_dict)
    device = predictor.model.arena.device
    gen = PromptGen(coco, num_points=num_points, num_neg_points=num_neg_points, include_center=include_center,
                    on_device=prompts_on_device, device=device)
    prompt_log: List[PromptInfo] = []
    segments = process_all_videos(predictor, gen, PROMPT_TYPES.get(prompt_type, prompt_type), clip_length,
                                  variable_cats, probs_out_dir=probs_out_dir, prompt_log=prompt_log,
                                  export_on_device=export_on_device, threshold=threshold, sweep=sweep,
                                  num_correction_clicks=num_correction_clicks, correction_method=correction_method,
                                  clicks_on_device=clicks_on_device)
    frames_by_video = {video_id: coco.frames(video_id) for video_id in coco.video_ids()}
    paths = save_as_coco_format(segments, frames_by_video, coco.mod, eval_dir, prompt_info=prompt_log,
                                save_video_list=save_video_list)
    if probs_out_dir is not None:
        from .tune_threshold import write_meta
        write_meta(probs_out_dir, coco.mod)
    return paths
