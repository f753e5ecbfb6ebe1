"""Threshold tuning -- sam2_video/eval/tune_threshold.py of the reference, from a probability dump (the
reference's way, kept as the A/B path and the tests' oracle) and from the device sweep (csrc/rle.hip
s2h_mask_sweep), which needs no dump.

The reference binarises float16 probabilities: a pixel of logit v counts at threshold t when
float16(sigmoid(v)) >= float16(t).  With h = float16(t), lo = the float16 below h and mid = (h + lo) / 2, that
is sigmoid(v) > mid, or >= mid when the tie at mid rounds to h (h's last mantissa bit is 0): a comparison of v
with one constant, `logit_cuts`.  The contract of the device path is `pixel counts at t <=> v >= cut(t)`, NaN
never counting: exact in integers and independent of anybody's expf.  A float32 torch.sigmoid followed by a
float16 rounding flips within a few float32 steps of the cut (hundreds at t = 0.5, where the float32 sigmoid is
coarse in v); pixels with |sigmoid(v) - mid| <= 2^-22 are where the two formulations may differ.

All K thresholds of a frame are one histogram: per category the pixelwise maximum logit m over its objects
falls into bin b = #{k : m >= cut_k}, split by the ground-truth bit.  The pixels predicted at threshold k are
the bins above k (suffix sums), the intersection the same sums over the ground-truth row: SweepAccumulator
turns the [ncat, 2, K + 1] integers of a frame into the reference's Dice sums.

Restated under the reference's names: grid_search (:26-131), dice_score (:12-15, on counts here), main
(:135-177).  No loguru or pycocotools: masks come through data/rle.py, `coco` is a path or the loaded dict.
"""
from __future__ import annotations

import argparse
import json
import math
import os
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np

from ..data import rle

AMBIGUOUS_BAND = 2.0 ** -22  # |sigmoid(v) - mid| up to which a float32 sigmoid may land on either side


def threshold_grid(t_min: float = 0.2, t_max: float = 0.8, t_step: float = 0.05) -> List[float]:
    """the reference's loop (:46-50): float accumulation, round(t, 5), <= t_max + 1e-9"""
    if not t_step > 0:
        raise ValueError(f"t_step must be positive, got {t_step}")
    thresholds = []
    t = t_min
    while t <= t_max + 1e-9:
        thresholds.append(round(t, 5))
        t += t_step
    return thresholds


def _check_thresholds(thresholds: Sequence[float]) -> List[float]:
    ts = [float(t) for t in thresholds]
    for t in ts:
        if not (0.0 < t <= 1.0):  # (NaN fails too)
            raise ValueError(f"thresholds must lie in (0, 1], got {t}")
    return ts


def threshold_mid(t: float) -> Tuple[float, bool]:
    """(mid, inclusive): float16(p) >= float16(t)  <=>  p > mid, or p >= mid when `inclusive`, for a real p.
    A t that rounds to float16 zero gives (-inf, True): every probability counts."""
    h = np.float16(t)
    if h == 0:
        return -math.inf, True
    lo = np.nextafter(h, np.float16(-1.0))
    mid = (float(h) + float(lo)) / 2.0  # exact in float64
    inclusive = (int(h.view(np.uint16)) & 1) == 0  # round-to-nearest-even: the tie goes to the even one
    return mid, inclusive


def logit_cuts(thresholds: Sequence[float]) -> np.ndarray:
    """float32 [K]: cut(t) = the smallest float32 c with sigmoid(c) > mid (>= mid in the tie-inclusive case),
    sigmoid taken exactly, so that float16(sigmoid(v)) >= float16(t)  <=>  v >= cut(t)."""
    cuts = np.empty(len(thresholds), dtype=np.float32)
    for i, t in enumerate(_check_thresholds(thresholds)):
        mid, inclusive = threshold_mid(t)
        if mid == -math.inf:
            cuts[i] = -np.inf
            continue
        x = math.log(mid / (1.0 - mid))
        c = np.float32(x)
        if float(c) < x or (float(c) == x and not inclusive):
            c = np.nextafter(c, np.float32(np.inf))
        cuts[i] = c
    return cuts


def dice_score(inter, pred, gt):
    """the reference's Dice (:12-15) on pixel counts: 2 * inter / (pred + gt + 1e-7) in float64"""
    inter, pred, gt = (np.asarray(v, dtype=np.float64) for v in (inter, pred, gt))
    d = 2.0 * inter / (pred + gt + 1e-7)
    return float(d) if d.ndim == 0 else d


def load_coco(coco: Union[str, os.PathLike, Dict]) -> Dict:
    if isinstance(coco, dict):
        return coco
    with open(coco, "r") as f:
        return json.load(f)


def _anns_by_image(coco: Dict) -> Dict[int, List[Dict]]:
    out: Dict[int, List[Dict]] = {}
    for a in coco.get("annotations", []):
        out.setdefault(int(a["image_id"]), []).append(a)
    return out


def _ann_mask(a: Dict, H: int, W: int) -> np.ndarray:
    seg = rle._as_rle(a["segmentation"])
    if [int(v) for v in seg["size"]] != [H, W]:
        raise ValueError(f"annotation {a.get('id')} of image {a['image_id']} has size {list(seg['size'])}, "
                         f"the frame is {[H, W]}")
    return rle.decode(seg).astype(bool)


def _gt_masks(anns: List[Dict], cats: Sequence[int], H: int, W: int) -> Dict[int, np.ndarray]:
    """per category the OR of its annotations (:79-89); an empty mask where it has none"""
    out = {}
    for c in cats:
        merged = np.zeros((H, W), dtype=bool)
        for a in anns:
            if a["category_id"] == c:
                merged |= _ann_mask(a, H, W)
        out[c] = merged
    return out


def load_meta(probs_dir: str) -> Dict:
    meta_path = os.path.join(probs_dir, "meta.json")
    if not os.path.exists(meta_path):
        raise FileNotFoundError(f"meta.json not found in {probs_dir}")
    with open(meta_path, "r") as f:
        return json.load(f)


def write_meta(probs_dir: str, mod: int) -> str:
    """the meta.json the reference's inference() leaves beside the dumps: mod, the image ids, the dtype"""
    image_ids = sorted(int(Path(p).stem) for p in os.listdir(probs_dir) if p.endswith(".npz") and Path(p).stem.isdigit())
    path = os.path.join(probs_dir, "meta.json")
    with open(path, "w") as f:
        json.dump({"mod": int(mod), "image_ids": image_ids, "dtype": "float16"}, f)
    return path


def _dump_image_ids(probs_dir: str, meta: Dict) -> List:
    image_ids = meta.get("image_ids")
    if not image_ids:  # fallback: scan the directory
        image_ids = [int(Path(p).stem) for p in os.listdir(probs_dir) if p.endswith(".npz") and Path(p).stem.isdigit()]
    return image_ids


def _best(thresholds: List[float], sum_dice: np.ndarray, count: np.ndarray):
    """mean Dice per threshold (-inf without samples), the argmax, ties to the threshold closest to 0.5"""
    valid = count > 0
    if not valid.any():
        raise RuntimeError("No valid categories found for Dice computation.")
    mean_dice = np.full_like(sum_dice, fill_value=-np.inf, dtype=np.float64)
    mean_dice[valid] = sum_dice[valid] / count[valid]
    best_idx = int(np.argmax(mean_dice))
    best_candidates = np.where(mean_dice == mean_dice[best_idx])[0]
    if len(best_candidates) > 1:
        best_idx = min(best_candidates, key=lambda i: abs(thresholds[i] - 0.5))
    per_thr = [(float(thresholds[i]), float(mean_dice[i])) for i in range(len(thresholds)) if valid[i]]
    return float(thresholds[best_idx]), float(mean_dice[best_idx]), per_thr


def grid_search(probs_dir: str, coco, t_min: float = 0.2, t_max: float = 0.8, t_step: float = 0.05,
                exclude_background: bool = False) -> Tuple[float, float, List[Tuple[float, float]]]:
    """the reference's grid search over a dump: per image, threshold and category (predicted or in the
    ground truth, sorted) `np.any(probs[idx] >= thr)` against the OR of the category's annotations.
    -> (best threshold, its mean Dice, [(threshold, mean Dice)])"""
    by_image = _anns_by_image(load_coco(coco))
    meta = load_meta(probs_dir)
    mod = int(meta["mod"])
    thresholds = threshold_grid(t_min, t_max, t_step)
    sum_dice = np.zeros(len(thresholds), dtype=np.float64)
    count = np.zeros(len(thresholds), dtype=np.int64)
    for image_id in _dump_image_ids(probs_dir, meta):
        npz_path = os.path.join(probs_dir, f"{image_id}.npz")
        if not os.path.exists(npz_path):
            continue
        data = np.load(npz_path)
        probs, obj_ids = data["probs"], data["obj_ids"]  # [N, H, W] float16, [N]
        H = int(data["height"]) if "height" in data else probs.shape[1]
        W = int(data["width"]) if "width" in data else probs.shape[2]
        pred_cat_ids = set((obj_ids % mod).tolist()) if obj_ids.size > 0 else set()
        anns = by_image.get(int(image_id), [])
        categories = sorted(pred_cat_ids.union(a["category_id"] for a in anns))
        if exclude_background and 0 in categories:
            categories.remove(0)
        gt_masks = _gt_masks(anns, categories, H, W)
        for ti, thr in enumerate(thresholds):
            for c in categories:
                pred_indices = np.where((obj_ids % mod) == c)[0]
                if pred_indices.size == 0 and not gt_masks[c].any():
                    continue  # neither predicted nor present
                if pred_indices.size == 0:
                    pred_mask = np.zeros((H, W), dtype=bool)
                else:
                    pred_mask = np.any(probs[pred_indices, :, :] >= thr, axis=0)
                sum_dice[ti] += dice_score(np.logical_and(pred_mask, gt_masks[c]).sum(), pred_mask.sum(),
                                           gt_masks[c].sum())
                count[ti] += 1
    return _best(thresholds, sum_dice, count)


class SweepAccumulator:
    """grid_search without a dump: the frames' sweep histograms (MergedFrame.result()["sweep"]) in, the
    reference's (best threshold, best Dice, curve) out.

    thresholds ascending in (0, 1] (threshold_grid); `cuts` are their logit cuts, what the predictor's
    `sweep_cuts=` takes; `gt_bits` packs a frame's ground truth for the kernel.  Frames are summed in the
    order they are added, thresholds and sorted categories within a frame as the reference's loop does.  A
    frame without objects adds nothing: the reference writes no dump for it and skips the image."""

    def __init__(self, thresholds: Sequence[float], coco, mod: int, exclude_background: bool = False):
        self.thresholds = _check_thresholds(thresholds)
        if not self.thresholds or len(self.thresholds) > 64:
            raise ValueError("1 to 64 thresholds per sweep")
        if any(b < a for a, b in zip(self.thresholds, self.thresholds[1:])):
            raise ValueError("thresholds must ascend")
        self.cuts = logit_cuts(self.thresholds)
        self.mod, self.exclude_background = int(mod), bool(exclude_background)
        self._anns = _anns_by_image(load_coco(coco))
        self.sum_dice = np.zeros(len(self.thresholds), dtype=np.float64)
        self.count = np.zeros(len(self.thresholds), dtype=np.int64)
        self.frames = {}  # image_id -> the frame's histogram, for inspection (and the first-visit rule)

    def __contains__(self, image_id) -> bool:
        return int(image_id) in self.frames

    def gt_bits(self, image_id, cat_ids: Sequence[int], H: int, W: int) -> np.ndarray:
        """int64 [len(cat_ids), ceil(H W / 64)]: per category the OR of the image's annotations, bit-packed
        column-major (ops.pack_mask_bits).  ValueError when an annotation's size is not [H, W]."""
        from ..kernels.ops import pack_mask_bits
        masks = _gt_masks(self._anns.get(int(image_id), []), list(cat_ids), int(H), int(W))
        return pack_mask_bits(np.stack([masks[c] for c in cat_ids]) if len(cat_ids) else
                              np.zeros((0, int(H), int(W)), bool))

    def add_frame(self, image_id, obj_ids: Sequence[int], cat_ids: Sequence[int], hist) -> None:
        """hist int32 [len(cat_ids), 2, K + 1] of the frame, the categories in `cat_ids` order"""
        image_id = int(image_id)
        if image_id in self.frames:
            raise ValueError(f"image {image_id} was added before")
        K = len(self.thresholds)
        hist = np.asarray(hist).reshape(len(cat_ids), 2, K + 1).astype(np.int64)
        self.frames[image_id] = hist
        if len(obj_ids) == 0:
            return
        pred_cats = {int(o) % self.mod for o in obj_ids}
        if pred_cats != {int(c) for c in cat_ids}:
            raise ValueError(f"cat_ids {list(cat_ids)} are not the categories of obj_ids {list(obj_ids)}")
        anns = self._anns.get(image_id, [])
        categories = sorted(pred_cats.union(a["category_id"] for a in anns))
        if self.exclude_background and 0 in categories:
            categories.remove(0)
        index = {int(c): i for i, c in enumerate(cat_ids)}
        for c in categories:
            if c in index:
                h = hist[index[c]]
                # pixels at threshold k = the bins above k: suffix sums without the first bin
                pred = np.cumsum((h[0] + h[1])[::-1])[::-1][1:]
                inter = np.cumsum(h[1][::-1])[::-1][1:]
                d = dice_score(inter, pred, h[1].sum())
            else:  # in the ground truth only: an empty prediction, Dice 0, counted -- unless its mask is empty
                size = rle._as_rle(anns[0]["segmentation"])["size"]
                gt = _gt_masks(anns, [c], int(size[0]), int(size[1]))[c]
                if not gt.any():
                    continue
                d = dice_score(np.zeros(K), np.zeros(K), gt.sum())
            self.sum_dice += d
            self.count += 1

    def result(self) -> Tuple[float, float, List[Tuple[float, float]]]:
        return _best(self.thresholds, self.sum_dice, self.count)


def best_threshold_payload(best_thr, best_dice, per_thr, t_min, t_max, t_step, exclude_background) -> Dict:
    """the reference's best_threshold.json (:164-174)"""
    return {"best_threshold": best_thr, "best_dice": best_dice, "threshold_curve": per_thr,
            "exclude_background": bool(exclude_background),
            "range": {"min": float(t_min), "max": float(t_max), "step": float(t_step)}}


def main(argv: Optional[Sequence[str]] = None):
    parser = argparse.ArgumentParser(description="Grid search probability threshold for best Dice using saved probs")
    parser.add_argument("--probs-dir", required=True, type=str)
    parser.add_argument("--coco-path", required=True, type=str)
    parser.add_argument("--min", dest="t_min", type=float, default=0.2)
    parser.add_argument("--max", dest="t_max", type=float, default=0.8)
    parser.add_argument("--step", dest="t_step", type=float, default=0.05)
    parser.add_argument("--exclude-background", action="store_true")
    parser.add_argument("--output-json", type=str, default=None,
                        help="Path to save best_threshold.json (defaults to probs_dir/../best_threshold.json)")
    args = parser.parse_args(argv)
    best_thr, best_dice, per_thr = grid_search(args.probs_dir, args.coco_path, args.t_min, args.t_max, args.t_step,
                                               args.exclude_background)
    out_path = args.output_json or str(Path(args.probs_dir).parent / "best_threshold.json")
    with open(out_path, "w") as f:
        json.dump(best_threshold_payload(best_thr, best_dice, per_thr, args.t_min, args.t_max, args.t_step,
                                         args.exclude_background), f, indent=2)
    print(f"Saved best threshold {best_thr:.3f} (Dice={best_dice:.4f}) to {out_path}")
    return out_path


if __name__ == "__main__":
    main()
