"""Shared inputs and independent numpy / scipy models of the prompt-generation tests (test_gt_prompts_host.py runs
the host build of csrc/gtprompt.h on them, test_gt_prompts_gpu.py the kernels): a shift-and-OR/AND loop for the
morphology, rle.decode, scipy.ndimage.label with a 3 x 3 structure, np.argwhere.  Nothing here calls the
package's own new host path (eval/utils.py mask_to_masks / mask_to_points)."""
import functools
import json
import os

import numpy as np

import cc_patterns as cp
from sam2_video.data import rle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_RLE = os.path.join(ROOT, "tests", "golden", "rle_endovis18_sample.json")

DECODE_SHAPES = [(1, 1), (7, 9), (64, 1), (1, 64), (33, 65)]
MORPH_SHAPES = [(1, 1), (3, 17), (9, 9), (10, 10), (11, 23), (37, 41), (64, 130)]
WINDOWS = [((0, 0), (0, 0)), ((-1, 1), (-1, 1)), ((-5, 4), (-5, 4)), ((-4, 5), (-4, 5)), ((-2, 0), (0, 3))]  # (y, x)
COMP_SHAPES = [(1, 1), (1, 17), (17, 1), (2, 2), (37, 53), (65, 130)]  # of cc_patterns.SHAPES
GRID_SPACINGS = [None, 1, 3, 1000]
BIG = (1100, 1000)  # more than 2^20 pixels: several scan rounds per image, two chunks per thread in the rank pick


# ------------------------------------------------------------------------------------------------ decode
def decode_patterns(H, W):
    """name -> bool [H, W]"""
    yy, xx = np.mgrid[0:H, 0:W]
    out = {"empty": np.zeros((H, W), bool), "full": np.ones((H, W), bool), "first": np.zeros((H, W), bool),
           "last": np.zeros((H, W), bool), "checkerboard": (yy + xx) % 2 == 0,
           "random": np.random.default_rng(H * 131 + W).random((H, W)) < 0.4}
    out["first"][0, 0] = True
    out["last"][-1, -1] = True
    return out


def counts_of(mask):
    """uncompressed COCO counts of a bool mask (column-major runs, starting with zeros)"""
    return rle.counts_from_string(rle.encode(mask)["counts"])


def golden_annotations():
    """[(H, W, counts, decoded uint8 [H, W])] of tests/golden/rle_endovis18_sample.json"""
    found = []

    def walk(node):
        if isinstance(node, dict):
            if "counts" in node and "size" in node:
                found.append(node)
                return
            node = list(node.values())
        if isinstance(node, list):
            for v in node:
                walk(v)
        elif isinstance(node, str) and node.startswith("{") and "counts" in node:
            found.append(node)

    with open(GOLDEN_RLE) as f:
        walk(json.load(f))
    out = []
    for seg in found:
        seg = rle._as_rle(seg)
        c = seg["counts"]
        c = rle.counts_from_string(c.decode("ascii") if isinstance(c, bytes) else c) if not isinstance(c, list) else c
        out.append((int(seg["size"][0]), int(seg["size"][1]), list(c), rle.decode(seg)))
    return out


# ------------------------------------------------------------------------------------------------ morphology
def morph_model(m, op, y_win, x_win):
    """shift-and-OR (op 0) / shift-and-AND (op 1) over the window's offsets; positions outside the image are
    ignored (the neutral element is shifted in)"""
    m = np.asarray(m).astype(bool)
    H, W = m.shape
    out = np.full((H, W), bool(op))
    for dy in range(y_win[0], y_win[1] + 1):
        for dx in range(x_win[0], x_win[1] + 1):
            s = np.full((H, W), bool(op))
            y0, y1, x0, x1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
            if y0 < y1 and x0 < x1:
                s[y0:y1, x0:x1] = m[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
            out = (out & s) if op else (out | s)
    return out


def morph_patterns(H, W):
    out = {"empty": np.zeros((H, W), bool), "full": np.ones((H, W), bool), "corners_centre": np.zeros((H, W), bool),
           "p0.01": np.random.default_rng(H * 7 + W).random((H, W)) < 0.01,
           "p0.5": np.random.default_rng(H * 11 + W).random((H, W)) < 0.5}
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2, W // 2)):
        out["corners_centre"][y, x] = True
    return out


def close_model(m, dilate_window=(-5, 4), erode_window=(-5, 4)):
    return morph_model(morph_model(m, 0, dilate_window, dilate_window), 1, erode_window, erode_window)


# ------------------------------------------------------------------------------------------------ components
def make_grid(H, W, spacing):
    if spacing is None:
        return None
    g = np.zeros((H, W), bool)
    for y in range(0, H, spacing):
        for x in range(0, W, spacing):
            g[y, x] = True
    return g


def components_model(binary, min_area, grid=None):
    """-> (stats int64 [n, 9] of the components of area >= min_area in raster order of their first pixel: root
    label, area, xmin, ymin, xmax, ymax, n_sel, sum x, sum y; index int32 [H, W]: 0 or the component's 1-based
    number -- not clipped to a byte)"""
    canon, areas = cp.reference(np.asarray(binary).astype(bool))
    rows, index = [], np.zeros(canon.shape, np.int32)
    for lab in np.unique(canon[canon > 0]):  # ascending label = ascending first pixel
        m = canon == lab
        ys, xs = np.nonzero(m)
        if ys.size < min_area:
            continue
        sel = np.argwhere(m & grid) if grid is not None else np.argwhere(m)
        rows.append([int(lab), int(ys.size), xs.min(), ys.min(), xs.max(), ys.max(), len(sel), sel[:, 1].sum(),
                     sel[:, 0].sum()])
        index[m] = len(rows)
    return np.asarray(rows, np.int64).reshape(-1, 9), index


def area_cases():
    """a 40 x 40 image with isolated components of area 9, 10 and 11 (a 3 x 3 block, plus one and two pixels)"""
    m = np.zeros((40, 40), bool)
    m[2:5, 2:5] = True
    m[12:15, 20:23] = True
    m[15, 20] = True
    m[30:33, 5:8] = True
    m[33, 5:7] = True
    return m


@functools.lru_cache(maxsize=None)
def big_blobs():
    """BIG image of random rectangles: a few hundred components, some beyond the 2^20-th pixel"""
    H, W = BIG
    rng = np.random.default_rng(5)
    m = np.zeros((H, W), bool)
    for _ in range(150):
        y, x = int(rng.integers(0, H - 40)), int(rng.integers(0, W - 40))
        m[y:y + int(rng.integers(1, 40)), x:x + int(rng.integers(1, 40))] = True
    m[H - 3:, W - 7:] = True
    m.setflags(write=False)
    return m


# ------------------------------------------------------------------------------------------------ rank select
def rank_model(labels, q_label, neg, grid, rank):
    """-> ((x, y) of the rank-th selected pixel in np.argwhere order or (-1, -1), the number of selected pixels)"""
    sel = (labels == q_label) != bool(neg)
    if grid is not None:
        sel = sel & grid
    pts = np.argwhere(sel)
    if 0 <= rank < len(pts):
        return (int(pts[rank][1]), int(pts[rank][0])), len(pts)
    return (-1, -1), len(pts)


# ------------------------------------------------------------------------------------------------ shared cases
def component_cases():
    """[(name, binary [N, H, W], min_area, grid or None, capacity)]"""
    out = []
    for H, W in COMP_SHAPES:
        pats = cp.patterns(H, W)
        names = list(pats)
        for k, spacing in enumerate(GRID_SPACINGS):
            idx = [(3 * k + j) % len(names) for j in range(len(names))]  # every pattern, rotated per grid
            out.append((f"{H}x{W}_g{spacing}", np.stack([pats[names[i]] for i in idx]), 1 + 2 * k,
                        make_grid(H, W, spacing), 255 * len(idx)))
    for min_area in (9, 10, 11, 12):
        out.append((f"areas_{min_area}", area_cases()[None], min_area, None, 8))
    out.append(("capacity_2", np.stack([area_cases(), area_cases().T]), 1, make_grid(40, 40, 3), 2))
    out.append(("capacity_0", area_cases()[None], 1, None, 0))
    out.append(("big", big_blobs()[None], 10, make_grid(*BIG, 4), 255))
    return out


def check_components(name, binary, min_area, grid, capacity, hdr, stats, index):
    """hdr int32 [2 N + 2], stats int64 [rows >= min(total, capacity), 9], index uint8 [N, H, W] against the model"""
    N = binary.shape[0]
    models = [components_model(b, min_area, grid) for b in binary]
    counts = [len(s) for s, _ in models]
    offs = np.concatenate([[0], np.cumsum(counts)])
    assert list(hdr[0:2 * N:2]) == counts and list(hdr[1:2 * N:2]) == list(offs[:-1]), name
    assert hdr[2 * N] == offs[-1] and hdr[2 * N + 1] == int(max(counts, default=0) > 255), name
    want = np.concatenate([s for s, _ in models]) if N else np.zeros((0, 9), np.int64)
    n = min(len(want), capacity)
    assert np.array_equal(stats[:n], want[:n]), name
    for b in range(N):
        if counts[b] <= 255:
            assert np.array_equal(index[b], models[b][1].astype(np.uint8)), (name, b)
        else:  # saturated, flagged by the status word
            assert np.array_equal(index[b], np.minimum(models[b][1], 255).astype(np.uint8)), (name, b)
    return counts


def rank_cases():
    """[(name, labels int32 [N, H, W], grid, [(img, label, neg, rank)])]"""
    out = []
    rng = np.random.default_rng(3)
    for (H, W), names in (((1, 1), ["all_foreground"]), ((37, 53), ["rings", "noise_p0.5_s0"]),
                          ((65, 130), ["corner_blocks", "serpentine", "noise_p0.3_s1"]), ((9, 65), ["spiral"])):
        pats = cp.patterns(H, W)
        labels = np.stack([cp.reference(pats[k])[0] for k in names])
        for spacing in (None, 3):
            grid = make_grid(H, W, spacing)
            qs = []
            for img in range(len(names)):
                labs = np.unique(labels[img][labels[img] > 0])
                for lab in list(labs[:2]) + list(labs[-1:]) + [H * W + 5]:  # (the last: a label no pixel has)
                    for neg in (0, 1):
                        n = rank_model(labels[img], lab, neg, grid, 0)[1]
                        qs += [(img, int(lab), neg, r) for r in {0, n - 1, n // 2, n, -1, int(rng.integers(0, n + 1))}]
            qs += [(len(names), 1, 0, 0), (-1, 1, 1, 0)]  # an image index outside the batch: count 0
            out.append((f"{H}x{W}_g{spacing}", labels, grid, qs))
    big = cp.reference(big_blobs())[0]
    labs = np.unique(big[big > 0])
    qs = []
    for lab, neg in ((labs[0], 0), (labs[-1], 0), (labs[len(labs) // 2], 1), (labs[-1], 1)):
        n = rank_model(big, lab, neg, None, 0)[1]
        qs += [(0, int(lab), neg, r) for r in (0, n - 1, n // 2, n)]
    out.append(("big", big[None], None, qs))
    return out


def check_ranks(name, labels, grid, qs, xy, count):
    for (img, lab, neg, rank), got, c in zip(qs, xy, count):
        if 0 <= img < len(labels):
            want, n = rank_model(labels[img], lab, neg, grid, rank)
        else:
            want, n = (-1, -1), 0
        assert tuple(got) == want and c == n, (name, img, lab, neg, rank, tuple(got), want, c, n)


# ------------------------------------------------------------------------------------------------ prompts
def points_model(mask, grid, num_points, include_center):
    """the reference's mask_to_points (eval/utils.py:125-153) restated for the tests, the grid as an argument"""
    assert isinstance(mask, np.ndarray) and mask.dtype == bool
    pts = np.argwhere(mask & grid if grid is not None else mask)[:, [1, 0]]
    if include_center is True:
        centre = np.mean(pts, axis=0).astype(int).reshape(1, -1)
        num_points -= 1
    if num_points > pts.shape[0]:
        return pts
    picked = pts[np.random.choice(pts.shape[0], num_points, replace=False)]
    return np.concatenate([centre, picked], axis=0) if include_center else picked


def masks_model(raw, dilate_window=(-5, 4), min_area=10):
    """the reference's mask_to_masks with the closing as close_model: bool masks in raster order"""
    stats, index = components_model(close_model(raw, dilate_window), min_area)
    return [index == i + 1 for i in range(len(stats))]


def objs_model(anns, mod, obj_count, num_points, num_neg_points, include_center, grid):
    """get_each_obj (inference.py:275-326) on the models above -> ([(obj_id, bbox, points, labels, mask)], count)"""
    out = []
    for ann in anns:
        for mask in masks_model(rle.decode(ann["segmentation"])):
            pos = points_model(mask, grid, num_points, include_center)
            neg = points_model(~mask, grid, num_neg_points, False)
            ys, xs = np.nonzero(mask)
            out.append((obj_count * mod + ann["category_id"],
                        [float(xs.min()), float(ys.min()), float(xs.max()), float(ys.max())],
                        np.concatenate([pos, neg]), np.concatenate([np.ones(len(pos)), np.zeros(len(neg))]), mask))
            obj_count += 1
    return out, obj_count


def prompt_frame_case():
    """a 48 x 80 frame with three annotations in two categories; the first closes into two components and a
    speck below area 10 -> (coco dict, frame dict)"""
    H, W = 48, 80
    a = np.zeros((H, W), bool)
    a[5:15, 6:20] = True
    a[8:11, 24:30] = True     # 4 px from the block: the closing bridges it
    a[30:40, 50:64] = True    # far away: a second component
    a[40:42, 20:22] = True    # a speck of area 4, away from the border (where the closing would grow it)
    b = np.zeros((H, W), bool)
    b[20:28, 30:45] = True
    b[22:26, 34:40] = False   # a hole the closing fills
    c = np.zeros((H, W), bool)
    c[0:6, 70:80] = True      # touches the border
    anns = [{"id": i + 1, "image_id": 7, "category_id": cat, "segmentation": rle.encode(m), "iscrowd": 0}
            for i, (cat, m) in enumerate(((1, a), (2, b), (1, c)))]
    frame = {"id": 7, "video_id": "v", "order_in_video": 0, "height": H, "width": W, "path": "0.jpg",
             "is_det_keyframe": True}
    coco = {"images": [frame], "annotations": anns, "categories": [{"id": 1, "name": "a"}, {"id": 2, "name": "b"}]}
    return coco, frame


# ------------------------------------------------------------------------------------------------ offline scores
def eval_model(gt, predictions, cats):
    """the averages eval() should report, from the decoded masks: per keyframe and category the OR of each side's
    masks through caculate_iou / caculate_mae / caculate_dice, then nanmeans per frame -> video -> overall"""
    from sam2_video.eval import eval as E

    def nanmean(v):
        v = np.asarray(v, np.float64)
        return np.nan if v.size == 0 or np.all(np.isnan(v)) else float(np.nanmean(v))

    videos = {}
    for img in gt["images"]:
        if img.get("is_det_keyframe") is False:
            continue
        frame = {}
        for c in cats:
            side = []
            for anns in (predictions, gt["annotations"]):
                side.append(E.merge_masks([rle.decode(a["segmentation"]) for a in anns
                                           if a["image_id"] == img["id"] and a["category_id"] == c]))
            p, g = side
            if p is None and g is None:
                frame[c] = {k: np.nan for k in E.KEYS}
                continue
            p = np.zeros_like(g) if p is None else p
            g = np.zeros_like(p) if g is None else g
            frame[c] = {"iou": E.caculate_iou(p, g), "mae": E.caculate_mae(p, g), "dice": E.caculate_dice(p, g)}
        videos.setdefault(img["video_id"], []).append(frame)
    per_video = [{c: {k: nanmean([f[c][k] for f in frames]) for k in E.KEYS} for c in cats} for frames in videos.values()]
    overall = {c: {k: nanmean([v[c][k] for v in per_video]) for k in E.KEYS} for c in cats}
    return {k: nanmean([overall[c][k] for c in cats]) for k in E.KEYS}
