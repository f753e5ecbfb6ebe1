"""Evaluation metrics -- drop-in for sam2_video/eval/eval.py of the reference (IoU / Dice / MAE
of the category-merged binarised masks, aggregated per frame, per video and over videos).

The reference evaluates offline from COCO json (predictions written by inference.py:862-901,
one annotation per non-empty merged category mask).  Here the same numbers are computed in
the loop from the model's outputs: one HIP reduction per frame (s2h_mask_eval_counts) gives
|pred & gt|, |pred | gt|, |pred|, |gt| per category on the device, and the scores follow in
closed form from those integers:
    iou  = |p & g| / (|p | g| + 1e-7)                     caculate_iou   (eval.py:16-30)
    dice = 2 |p & g| / (|p| + |g| + 1e-7)                 caculate_dice  (eval.py:33-36)
    mae  = (|p & !g| + 255 |!p & g|) / P                  caculate_mae(dt, gt) on uint8
                                                          masks (eval.py:39-40, :102): dt - gt
                                                          wraps to 255 where dt = 0, gt = 1
A category with neither a predicted nor a ground-truth pixel has no annotation in either file
and is skipped (eval.py:85-86) -- NaN, ignored by the nanmeans.  The per-video and overall
aggregation (get_video_scores / get_result) is nanmean over at most a few dozen numbers, done on
the host.  The numpy helpers keep the reference's names and signatures.
"""
from __future__ import annotations

from typing import Dict, List, Sequence

import numpy as np
import torch

from ..kernels import ops

KEYS = ("iou", "mae", "dice")


# ---------------------------------------------------------- reference helpers (host, numpy)
def caculate_iou(pred, gt):
    """eval.py:16-30"""
    intersection = np.logical_and(pred, gt).sum()
    union = np.logical_or(pred, gt).sum() + 1e-7
    return intersection / union


def caculate_dice(pred, gt):
    """eval.py:33-36"""
    intersection = np.sum(pred * gt)
    return (2.0 * intersection) / (np.sum(pred) + np.sum(gt) + 1e-7)


def caculate_mae(y_true, y_pred):
    """eval.py:39-40"""
    return np.mean(np.abs(y_true - y_pred))


def merge_masks(masks):
    """eval.py:43-50"""
    if not masks:
        return None
    merged = np.zeros_like(masks[0])
    for m in masks:
        merged = np.logical_or(merged, m)
    return merged.astype(np.uint8)


def _nanmean(v):
    v = np.asarray(v, dtype=np.float64)
    return float(np.nanmean(v)) if v.size and not np.all(np.isnan(v)) else float("nan")


# ------------------------------------------------------------------ device path
def frame_counts(pred_logits: torch.Tensor, gt: torch.Tensor) -> torch.Tensor:
    """[N_cat, 4] int64 on the device: |p & g|, |p | g|, |p|, |g| with p = pred_logits > 0.
    pred_logits [N_cat, (1,) H, W] fp32 (category-merged high-res logits), gt [N_cat, H, W]."""
    return ops.mask_eval_counts(pred_logits.detach().contiguous(), gt.contiguous())


def image_scores_from_counts(counts, num_pixels: int, cat_ids: Sequence = None) -> Dict:
    """get_image_scores (eval.py:53-141) for one frame from the per-category counts."""
    c = np.asarray(counts, dtype=np.int64).reshape(-1, 4)
    cat_ids = list(range(c.shape[0])) if cat_ids is None else list(cat_ids)
    cat = {}
    for n, cid in enumerate(cat_ids):
        inter, union, npred, ngt = (int(v) for v in c[n])
        if npred == 0 and ngt == 0:
            cat[cid] = {k: float("nan") for k in KEYS}
            continue
        cat[cid] = {"iou": inter / (union + 1e-7),
                    "mae": ((npred - inter) + 255.0 * (ngt - inter)) / float(num_pixels),
                    "dice": (2.0 * inter) / (npred + ngt + 1e-7)}
    return {"cat_scores": cat, "avg_scores": {k: _nanmean([cat[i][k] for i in cat_ids]) for k in KEYS}}


def get_video_scores_from_frames(img_scores: List[Dict], cat_ids: Sequence) -> Dict:
    """get_video_scores (eval.py:144-206) for one video"""
    cat = {c: {k: _nanmean([f["cat_scores"][c][k] for f in img_scores]) for k in KEYS} for c in cat_ids}
    return {"frames": img_scores, "cat_scores": cat,
            "avg_scores": {k: _nanmean([cat[c][k] for c in cat_ids]) for k in KEYS}}


def get_result(video_scores: List[Dict], cat_ids: Sequence) -> Dict:
    """get_result (eval.py:209-258)"""
    cat = {c: {k: _nanmean([v["cat_scores"][c][k] for v in video_scores]) for k in KEYS} for c in cat_ids}
    return {"videos": video_scores, "cat_scores": cat,
            "avg_scores": {k: _nanmean([cat[c][k] for c in cat_ids]) for k in KEYS}}


@torch.no_grad()
def evaluate_clip(merged_frames: List[Dict], target_masks: torch.Tensor, cat_ids: Sequence = None) -> Dict:
    """Scores of one clip from SAM2Model.forward's category-merged outputs (pred_masks_high_res
    [N_cat, 1, H, W] per frame) against its masks [T, N_cat, H, W]: the video-level dict of
    get_video_scores, every frame counted (synthetic clips have no non-keyframes)."""
    T = len(merged_frames)
    counts = torch.stack([frame_counts(f["pred_masks_high_res"], target_masks[t]) for t, f in enumerate(merged_frames)])
    counts = counts.cpu().numpy()  # one device->host copy per clip
    n_cat = counts.shape[1]
    cat_ids = list(range(n_cat)) if cat_ids is None else list(cat_ids)
    P = int(target_masks[0, 0].numel())
    frames = [image_scores_from_counts(counts[t], P, cat_ids) for t in range(T)]
    return get_video_scores_from_frames(frames, cat_ids)


# ------------------------------------------------------------------ offline scoring (host, numpy)
def _merged_counts(anns_dt, anns_gt):
    """|p & g|, |p | g|, |p|, |g| and the pixel count of the OR-ed masks of one category (eval.py:88-103)"""
    from ..data import rle
    dt = merge_masks([rle.decode(a["segmentation"]) for a in anns_dt])
    gt = merge_masks([rle.decode(a["segmentation"]) for a in anns_gt])
    if dt is None:
        dt = np.zeros_like(gt)
    if gt is None:
        gt = np.zeros_like(dt)
    p, g = dt.astype(bool), gt.astype(bool)
    return [int((p & g).sum()), int((p | g).sum()), int(p.sum()), int(g.sum())], p.size


def _device_counts(images, by_image, cat_ids, device="cuda"):
    """{(image id, category id): (the four counts, pixel count)} for every (image, category) group with an
    annotation on either side, counted on the device from the run boundaries (ops.rle_pair_counts:
    s2h_rle_pair_counts) -- the groups batched by mask size, one launch per size (split where a batch would pass
    the kernel's G H W < 2^31 limit); nothing is decoded on the host and only the runs are uploaded"""
    from ..data import rle
    batches: Dict = {}
    for img in images:
        anns_dt, anns_gt = by_image["dt"].get(img["id"], []), by_image["gt"].get(img["id"], [])
        for c in cat_ids:
            sides = [[rle.counts_of(a["segmentation"]) for a in anns if a["category_id"] == c]
                     for anns in (anns_dt, anns_gt)]
            if not sides[0] and not sides[1]:
                continue
            shapes = {(h, w) for side in sides for h, w, _ in side}
            if len(shapes) != 1:
                raise ValueError(f"image {img['id']}, category {c}: annotation masks of sizes {sorted(shapes)}")
            keys, dts, gts = batches.setdefault(shapes.pop(), ([], [], []))
            keys.append((img["id"], c))
            dts.append([cnts for _, _, cnts in sides[0]])
            gts.append([cnts for _, _, cnts in sides[1]])
    out = {}
    for (h, w), (keys, dts, gts) in batches.items():
        step = max(1, (2 ** 31 - 257) // (h * w))
        for i in range(0, len(keys), step):
            counts = ops.rle_pair_counts(dts[i:i + step], gts[i:i + step], h, w, device=device).cpu().numpy()
            for key, row in zip(keys[i:i + step], counts):
                out[key] = ([int(v) for v in row], h * w)
    return out


def eval(predict_path, coco_path, output_path, remove_background=False, *,  # noqa: A001 (the reference's name)
         score_on_device=None):
    """eval.py:53-277 without pycocotools: score `predict_path` (the annotation list inference() writes) against
    the ground-truth COCO file and write `<output_path>/eval.pkl` -- {"videos": [{"video_id", "frames": [{"video_id",
    "order_in_video", "cat_scores", "avg_scores"}], "cat_scores", "avg_scores"}], "cat_scores", "avg_scores"} with
    iou / mae / dice per category id of the ground-truth file (without 0 when remove_background).  -> the result.

    Only images whose is_det_keyframe is not False are scored.  Per category the annotations of each side are
    OR-ed (data/rle.py decodes them); a category with no annotation on either side is skipped (NaN, ignored by
    the nanmeans); the four counts go through image_scores_from_counts, whose closed forms are caculate_iou /
    caculate_dice / caculate_mae on the uint8 masks.  (One corner differs: annotations that exist on both sides
    but are all empty score NaN here and 0 in the reference; neither inference() nor a COCO export writes empty
    masks.)  Videos are listed in first-seen order (the reference iterates a set).

    score_on_device (None: True when torch.cuda.is_available()): the four counts of every (image, category) group
    come from s2h_rle_pair_counts, straight from the run boundaries (_device_counts), instead of the host's
    decode / OR / sum; the same integers go through the same image_scores_from_counts, so eval.pkl is identical.
    False: host numpy throughout."""
    import json
    import os
    import pickle
    with open(coco_path, "r") as f:
        gt = json.load(f)
    with open(predict_path, "r") as f:
        predictions = json.load(f)
    if isinstance(predictions, dict):
        predictions = predictions.get("annotations", [])
    cat_ids = [c["id"] for c in gt.get("categories", [])]
    if remove_background:
        cat_ids.remove(0)
    by_image = {"dt": {}, "gt": {}}
    for side, anns in (("dt", predictions), ("gt", gt.get("annotations", []))):
        for a in anns:
            by_image[side].setdefault(a["image_id"], []).append(a)
    if score_on_device is None:
        score_on_device = torch.cuda.is_available()
    on_device = None
    if score_on_device:
        on_device = _device_counts([i for i in gt.get("images", []) if i.get("is_det_keyframe") is not False],
                                   by_image, cat_ids)
    img_scores: List[Dict] = []
    for img in gt.get("images", []):
        if img.get("is_det_keyframe") is False:
            continue
        anns_dt, anns_gt = by_image["dt"].get(img["id"], []), by_image["gt"].get(img["id"], [])
        counts, num_pixels = [], int(img.get("height", 0)) * int(img.get("width", 0))
        for c in cat_ids:
            c_dt = [a for a in anns_dt if a["category_id"] == c]
            c_gt = [a for a in anns_gt if a["category_id"] == c]
            if not c_dt and not c_gt:
                counts.append([0, 0, 0, 0])
                continue
            row, num_pixels = on_device[(img["id"], c)] if on_device is not None else _merged_counts(c_dt, c_gt)
            counts.append(row)
        score = {"video_id": img["video_id"], "order_in_video": img["order_in_video"]}
        score.update(image_scores_from_counts(np.asarray(counts, dtype=np.int64).reshape(-1, 4), max(num_pixels, 1),
                                              cat_ids))
        img_scores.append(score)
    video_scores = []
    for video_id in dict.fromkeys(s["video_id"] for s in img_scores):
        video = {"video_id": video_id}
        video.update(get_video_scores_from_frames([s for s in img_scores if s["video_id"] == video_id], cat_ids))
        video_scores.append(video)
    result = get_result(video_scores, cat_ids)
    os.makedirs(str(output_path), exist_ok=True)
    with open(f"{output_path}/eval.pkl", "wb") as f:
        pickle.dump(result, f)
    return result
