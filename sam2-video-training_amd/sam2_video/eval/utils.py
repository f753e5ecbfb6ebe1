"""The evaluation's prompt types -- sam2_video/eval/utils.py of the reference, restated under its names:
ClipRange, PromptObj and PromptInfo with the reference's fields (utils.py:10-38), the two list helpers,
mask_to_bbox (utils.py:156-165) and the prompt generation from ground truth: init_grid / GRID, mask_to_points
(utils.py:116-153) and mask_to_masks (utils.py:95-113).  cv2 is not a dependency: mask_to_masks is the host path
in numpy / scipy (a rectangular closing whose window is the named constant below, 8-connected components in
raster order, area >= 10); eval/inference.py get_each_obj runs the same steps on the device (csrc/gtprompt.hip)
and keeps this one as its A/B path.  The plotting helpers are not restated (matplotlib / natsort are not
dependencies either).  mask_to_bbox also serves the threshold tuning's host path
(eval/export_predict_from_probs.py; the tuning itself is eval/tune_threshold.py)."""
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


# The closing of mask_to_masks (utils.py:95-99) is cv2.morphologyEx(mask, MORPH_CLOSE, ones((10, 10))) with the
# default anchor and border: a dilation followed by an erosion, both ignoring the pixels outside the image.
# OpenCV's documented formulas read the SAME offsets (x' - anchor) for both operations,
#     dilate: dst(x, y) = max over (x', y') of src(x + x' - anchor.x, y + y' - anchor.y)      erode: min over the same,
# and the default anchor of an even window of 10 is 5: the offsets -5 .. 4 along either axis, for both.  These
# constants hold (lo, hi) of that offset range, used for rows and columns alike.
# cv2 is not a dependency of this package or of its tests, but the reference's own data settles the reading:
# the 1285 masks its cv2.MORPH_OPEN with ones((10, 10)) wrote (data/endovis18_coco_annotations_val_opened.json)
# are shifted by +1 in x and y against their pre-opening boxes, and are fixed points of
# dilate(-5 .. 4) after erode(-4 .. 5) but not of dilate(-4 .. 5) after it at the image border -- DESIGN.md §9,
# "Dataset preparation on the device"; tests/test_dataprep_host.py pins it on 24 of them.
# The alternative reading -- a dilation by the REFLECTED window, offsets -4 .. 5, as the set-theoretic definition
# of a Minkowski sum has it -- is CLOSE_DILATE_WINDOW = (-4, 5).  Away from the image border the two give the
# same closed masks shifted by one pixel: the alternative's result is the default's moved by (-1, -1) in (x, y)
# (with the default windows a lone pixel at (y, x) closes to (y + 1, x + 1), with (-4, 5) to itself).  Everything
# else in mask_to_masks is independent of that choice; tests/test_gt_prompts_host.py has the cv2 comparison that
# settles it wherever cv2 exists.
CLOSE_DILATE_WINDOW = (-5, 4)
CLOSE_ERODE_WINDOW = (-5, 4)
MIN_COMPONENT_AREA = 10  # utils.py:105

GRID = None


def _window_counts(m, lo, hi, axis):
    """per position the number of set elements, and of in-image positions, among offsets lo .. hi along `axis`"""
    n = m.shape[axis]
    idx = np.arange(n)
    a, b = np.clip(idx + lo, 0, n), np.clip(idx + hi + 1, 0, n)
    cs = np.concatenate([np.zeros_like(np.take(m, [0], axis=axis), dtype=np.int64), np.cumsum(m, axis=axis, dtype=np.int64)],
                        axis=axis)
    shape = [1] * m.ndim
    shape[axis] = n
    return np.take(cs, b, axis=axis) - np.take(cs, a, axis=axis), (b - a).reshape(shape)


def rect_dilate(mask, y_win, x_win):
    """out(y, x) = OR of mask(y + dy, x + dx), dy in [y_win[0], y_win[1]], dx likewise, inside the image (host)"""
    m = np.asarray(mask).astype(bool)
    for axis, (lo, hi) in ((1, x_win), (0, y_win)):
        m = _window_counts(m, lo, hi, axis)[0] > 0
    return m


def rect_erode(mask, y_win, x_win):
    """out(y, x) = AND of mask(y + dy, x + dx) over the window's positions inside the image (host)"""
    m = np.asarray(mask).astype(bool)
    for axis, (lo, hi) in ((1, x_win), (0, y_win)):
        cnt, size = _window_counts(m, lo, hi, axis)
        m = cnt == size
    return m


def close_mask(mask, dilate_window=None, erode_window=None):
    """the 10 x 10 closing of mask_to_masks on the host (see CLOSE_DILATE_WINDOW)"""
    dw = CLOSE_DILATE_WINDOW if dilate_window is None else dilate_window
    ew = CLOSE_ERODE_WINDOW if erode_window is None else erode_window
    return rect_erode(rect_dilate(mask, dw, dw), ew, ew)


def label_components(binary):
    """8-connected components numbered 1 .. n in raster order of their first pixel
    (cv2.connectedComponentsWithStats' order) -> (labels int32 [H, W], areas int64 [n])"""
    from scipy import ndimage
    lab, n = ndimage.label(binary, structure=np.ones((3, 3), dtype=np.int32))
    if n == 0:
        return lab.astype(np.int32), np.zeros(0, np.int64)
    first = np.full(n + 1, lab.size, dtype=np.int64)
    flat = lab.ravel()
    np.minimum.at(first, flat, np.arange(flat.size))
    order = np.argsort(first[1:], kind="stable")  # scipy's number - 1 of the components, by first pixel
    renum = np.zeros(n + 1, dtype=np.int32)
    renum[order + 1] = np.arange(1, n + 1, dtype=np.int32)
    return renum[lab], np.bincount(flat, minlength=n + 1)[1:][order].astype(np.int64)


def mask_to_masks(mask: np.ndarray) -> list:
    """utils.py:95-113 on the host, numpy / scipy: close with a 10 x 10 window, 8-connected components in raster
    order, keep those of area >= 10 -> the bool masks `labels == i` of the CLOSED mask"""
    closed = close_mask(np.asarray(mask) != 0)
    labels, areas = label_components(closed)
    return [labels == i + 1 for i in range(areas.size) if areas[i] >= MIN_COMPONENT_AREA]


def init_grid(size, grid_spacing):
    """utils.py:116-122: GRID = bool [size] set at every grid_spacing-th row and column"""
    global GRID
    grid = np.zeros(size, dtype=bool)
    grid[0:size[0]:grid_spacing, 0:size[1]:grid_spacing] = True
    GRID = grid


def mask_to_points(mask, num_points=0, include_center=False):
    """utils.py:125-153, quirks included: (x, y) points of the mask (on the GRID when one is set); with the
    centre, `mean(points).astype(int)` comes first and takes one of the num_points; more points asked than
    there are returns them all WITHOUT the centre; the sample is np.random.choice(n, num_points, replace=False)
    of the global generator (so num_points = 0 with the centre asks for -1 points and raises)"""
    if not isinstance(mask, np.ndarray) or mask.dtype != bool:
        raise ValueError("mask must be a binary numpy array")
    points = np.argwhere(mask & GRID) if GRID is not None else np.argwhere(mask)
    points = points[:, [1, 0]]
    if include_center is True:
        center = np.mean(points, axis=0).astype(int).reshape(1, -1)
        num_points -= 1
    if num_points > points.shape[0]:
        return points
    sampled_points = points[np.random.choice(points.shape[0], num_points, replace=False)]
    if include_center:
        sampled_points = np.concatenate([center, sampled_points], axis=0)
    return sampled_points


def mask_to_bbox(mask):
    """corners [xmin, ymin, xmax, ymax] (inclusive, floats) of a binary mask, None when it is empty
    (utils.py:156-165; not COCO xywh)"""
    ys, xs = np.nonzero(np.asarray(mask))
    if ys.size == 0:
        return None
    return [float(xs.min()), float(ys.min()), float(xs.max()), float(ys.max())]
