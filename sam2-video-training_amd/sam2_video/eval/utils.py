"""The evaluation's prompt types -- sam2_video/eval/utils.py of the reference, restated under its names:
ClipRange, PromptObj and PromptInfo with the reference's fields (utils.py:10-38), the two list helpers and
mask_to_bbox (utils.py:156-165).  The plotting helpers and the prompt generation from ground truth
(mask_to_masks: cv2 closing + connected components, mask_to_points) are not restated: cv2 / matplotlib /
natsort are not dependencies of this package (see eval/inference.py).  mask_to_bbox also serves the threshold
tuning's host path (eval/export_predict_from_probs.py; the tuning itself is eval/tune_threshold.py)."""
from __future__ import annotations

from dataclasses import dataclass
from typing import List

import numpy as np


@dataclass
class ClipRange:
    """first and last frame of a clip, as `order_in_video` (inclusive)"""

    start_idx: int
    end_idx: int


@dataclass
class PromptObj:
    """one prompted object: whichever of mask / bbox / points the prompt type uses"""

    mask: np.ndarray
    bbox: List[float]
    points: List[List[float]]
    obj_id: int
    pos_or_neg_label: List[int]


@dataclass
class PromptInfo:
    """the prompts of one frame of a clip"""

    prompt_objs: List[PromptObj]
    frame_idx: int
    prompt_type: str
    video_id: str
    path: str
    clip_range: ClipRange


def get_dicts_by_field_value(data, field_name, target_value):
    return [item for item in data if item.get(field_name) == target_value]


def sort_dicts_by_field(data, field_name, reverse=False):
    """(the reference sorts with natsort; on the integer `order_in_video` this is the same order)"""
    return sorted(data, key=lambda item: item.get(field_name), reverse=reverse)


def mask_to_bbox(mask):
    """corners [xmin, ymin, xmax, ymax] (inclusive, floats) of a binary mask, None when it is empty
    (utils.py:156-165; not COCO xywh)"""
    ys, xs = np.nonzero(np.asarray(mask))
    if ys.size == 0:
        return None
    return [float(xs.min()), float(ys.min()), float(xs.max()), float(ys.max())]
