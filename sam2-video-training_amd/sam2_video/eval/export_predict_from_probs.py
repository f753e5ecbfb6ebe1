"""predict_t0.xx.json from a probability dump -- sam2_video/eval/export_predict_from_probs.py of the reference
(export_predict :22-92), restated without loguru or pycocotools (the RLE codec is data/rle.py).  The host A/B
path of `predict_on_video(threshold=...)` + `save_thresholded_predict` (eval/inference.py), which write the same
file from the device export without a dump.

Per dumped frame and category (`obj_id % mod`, in first-seen order of the frame's objects): the float16
probabilities thresholded with `>=`, OR-ed over the category's objects; empty masks are skipped; the score is
the category's maximum float16 probability.
"""
from __future__ import annotations

import argparse
import json
import os
from pathlib import Path
from typing import Dict, List, Optional, Sequence

import numpy as np

from ..data import rle
from .tune_threshold import _dump_image_ids, load_meta
from .utils import mask_to_bbox


def export_predict(probs_dir: str, threshold: float, output_predict: Optional[str] = None,
                   exclude_background: bool = False) -> str:
    meta = load_meta(probs_dir)
    mod = int(meta["mod"])
    annotations: List[Dict] = []
    for image_id in _dump_image_ids(probs_dir, meta):
        npz_path = os.path.join(probs_dir, f"{image_id}.npz")
        if not os.path.exists(npz_path):
            continue
        data = np.load(npz_path)
        probs, obj_ids = data["probs"], data["obj_ids"]  # [N, H, W] float16, [N]
        cat_to_indices: Dict[int, List[int]] = {}
        for idx, oid in enumerate(obj_ids.tolist()):
            cat_id = int(oid % mod)
            if exclude_background and cat_id == 0:
                continue
            cat_to_indices.setdefault(cat_id, []).append(idx)
        for cat_id, indices in cat_to_indices.items():
            merged = np.any(probs[np.asarray(indices, dtype=np.int64), :, :] >= threshold, axis=0)
            if merged.sum() == 0:
                continue
            score = float(np.max([float(probs[i].max()) for i in indices]))
            annotations.append({"image_id": int(image_id), "category_id": int(cat_id),
                                "segmentation": rle.encode(merged), "bbox": mask_to_bbox(merged), "iscrowd": 0,
                                "score": score})
    if output_predict is None:
        output_predict = str(Path(probs_dir).parent / f"predict_t{threshold:.2f}.json")
    with open(output_predict, "w") as f:
        json.dump(annotations, f, indent=2)
    return output_predict


def main(argv: Optional[Sequence[str]] = None):
    parser = argparse.ArgumentParser(description="Export predict.json from saved per-frame probability maps")
    parser.add_argument("--probs-dir", required=True, type=str)
    parser.add_argument("--threshold", required=True, type=float)
    parser.add_argument("--output-predict", type=str, default=None)
    parser.add_argument("--exclude-background", action="store_true")
    args = parser.parse_args(argv)
    path = export_predict(args.probs_dir, args.threshold, args.output_predict, args.exclude_background)
    print(f"Wrote predictions to {path}")
    return path


if __name__ == "__main__":
    main()
