"""The shared cases of the visualisation compositor (s2h_viz_pack / s2h_viz_compose, csrc/viz_host_check.cpp,
sam2_video/utils/viz.py) and an independent numpy / scipy model of the picture DESIGN.md section 9 defines:
float64 numpy for the frame conversion, np.rint(0.8 b + 0.2 o) for the blend, scipy's binary dilation / erosion
for the contour band, plain loops for the markers.  It shares no code with csrc/viz_pixel.h or with the package's
numpy path.

A case is a dict: name, n, C, H, W, step (the frame stride in frames: case frame f is stored frame f * step),
frames / gt / pred (stored arrays, (n - 1) step + 1 frames), frame0, prompt ([C, H, W] or None), markers int32
[M, 8] = {kind, x1, y1, x2, y2, r, g, b}, palette uint8 [C, 3].  Frames are fp32 [.., 3, H, W] or uint8
[.., H, W, 3]; masks are uint8 or fp32 [.., C, H, W]."""
import colorsys

import numpy as np
from scipy import ndimage

MEAN = np.array([0.485, 0.456, 0.406])
STD = np.array([0.229, 0.224, 0.225])
# not multiples of 4 or 64 (the compositor takes four pixels per lane, 256 lanes per workgroup), one pixel, and
# more than one workgroup
SIZES = [(1, 1), (5, 7), (17, 33), (64, 64), (130, 66)]
DISC, CROSS, BOX = 0, 1, 2
SPECIAL_LOGITS = np.array([0.5, np.nextafter(np.float32(0.5), np.float32(1)), 0.0, -0.0, np.inf, -np.inf], np.float32)


def palette_of(C):
    return np.array([[int(255 * v) for v in colorsys.hsv_to_rgb(c / C, 0.9, 0.9)] for c in range(C)], np.uint8)


# ------------------------------------------------------------------------------------------------ the model
def frame_u8(frames):
    """fp32 [n, 3, H, W] -> uint8 [n, H, W, 3] as the reference converts (viz.py:46-54); uint8 passes through"""
    if frames.dtype == np.uint8:
        return frames
    img = frames.transpose(0, 2, 3, 1)
    img = img * STD + MEAN  # float32 * float64 -> float64, two roundings
    img = np.clip(img, 0, 1)
    return (img * 255).astype(np.uint8)


def blend(base, over):
    return np.rint(base.astype(np.float64) * 0.8 + over.astype(np.float64) * 0.2).astype(np.uint8)


def overlay_panel(base, mask, palette):
    """base uint8 [H, W, 3], mask [C, H, W] of either kind"""
    bits = mask > 0.5
    over = np.zeros_like(base)
    for c in range(bits.shape[0]):
        over[bits[c]] = palette[c]
    out = blend(base, over)
    box = np.ones((3, 3), bool)
    for c in range(bits.shape[0]):
        grown = ndimage.binary_dilation(bits[c], structure=box, border_value=0)
        shrunk = ndimage.binary_erosion(bits[c], structure=box, border_value=1)
        out[grown & ~shrunk] = palette[c]
    return out


def draw_markers(img, markers):
    H, W = img.shape[:2]
    for kind, x1, y1, x2, y2, r, g, b in (tuple(int(v) for v in m) for m in markers):
        if kind == BOX:
            for y in range(max(y1, 0), min(y2, H - 1) + 1):
                for x in range(max(x1, 0), min(x2, W - 1) + 1):
                    if min(x - x1, x2 - x, y - y1, y2 - y) < 2:
                        img[y, x] = (r, g, b)
            continue
        for y in range(max(y1 - 9, 0), min(y1 + 9, H - 1) + 1):
            for x in range(max(x1 - 9, 0), min(x1 + 9, W - 1) + 1):
                dx, dy = x - x1, y - y1
                if kind == DISC:
                    d2 = dx * dx + dy * dy
                    if d2 < 49:
                        img[y, x] = (r, g, b)
                    elif d2 <= 81:
                        img[y, x] = (255, 255, 255)
                elif kind == CROSS:
                    if (abs(dx) <= 1 and abs(dy) <= 8) or (abs(dy) <= 1 and abs(dx) <= 8):
                        img[y, x] = (r, g, b)
    return img


def composites(frames, frame0, gt, pred, palette, markers=None, prompt=None):
    """frames [n, ..], gt / pred [n, C, H, W], frame0 one frame -> uint8 [n, 2H, 2W, 3]"""
    fu8, f0 = frame_u8(frames), frame_u8(frame0[None])[0]
    n, H, W = fu8.shape[:3]
    if prompt is not None:
        bl = overlay_panel(f0, prompt, palette)
    else:
        bl = draw_markers(f0.copy(), markers if markers is not None else [])
    out = np.empty((n, 2 * H, 2 * W, 3), np.uint8)
    for f in range(n):
        out[f] = np.concatenate([np.concatenate([fu8[f], overlay_panel(fu8[f], gt[f], palette)], axis=1),
                                 np.concatenate([bl, overlay_panel(fu8[f], pred[f], palette)], axis=1)], axis=0)
    return out


def reference(case):
    s = case["step"]
    return composites(case["frames"][::s], case["frame0"], case["gt"][::s], case["pred"][::s], case["palette"],
                      case["markers"], case["prompt"])


def markers_from_points(coords, labels, obj_to_cat, palette):
    """the marker table of frame 0's point inputs (viz.py:155-210): int() truncation, a disc per label 1, a cross
    per label 0; with a label 2 or 3 anywhere one box per object"""
    coords, labels = np.asarray(coords, np.float64), np.asarray(labels)
    is_box = bool(np.isin(labels, (2, 3)).any())
    rows = []
    for o in range(labels.shape[0]):
        col = [int(v) for v in palette[obj_to_cat[o]]]
        if is_box:
            c = [0, 0, 0, 0]
            for p in range(labels.shape[1]):
                if labels[o, p] == 2:
                    c[0], c[1] = int(coords[o, p, 0]), int(coords[o, p, 1])
                if labels[o, p] == 3:
                    c[2], c[3] = int(coords[o, p, 0]), int(coords[o, p, 1])
            rows.append([BOX] + c + col)
        else:
            for p in range(labels.shape[1]):
                if labels[o, p] == 1:
                    rows.append([DISC, int(coords[o, p, 0]), int(coords[o, p, 1]), 0, 0] + col)
                elif labels[o, p] == 0:
                    rows.append([CROSS, int(coords[o, p, 0]), int(coords[o, p, 1]), 0, 0] + col)
    return np.asarray(rows, np.int32).reshape(-1, 8)


# ------------------------------------------------------------------------------------------------ the cases
def patterns(H, W):
    """named bool [H, W] masks: empty, full, checkerboard, a 1-pixel hole, diagonal lines, blocks touching each
    border and each corner"""
    ys, xs = np.mgrid[0:H, 0:W]
    bh, bw = max(1, H // 3), max(1, W // 3)
    hole = np.ones((H, W), bool)
    hole[H // 2, W // 2] = False
    out = {"empty": np.zeros((H, W), bool), "full": np.ones((H, W), bool), "checker": (ys + xs) % 2 == 0, "hole": hole,
           "diag": ((ys - xs) % 5 == 0) | ((ys + xs) % 7 == 0),
           "top": (ys < bh) & (xs >= bw) & (xs < W - bw) if W > 2 * bw else ys < bh,
           "bottom": ys >= H - bh, "left": xs < bw, "right": (xs >= W - bw) & (ys >= bh),
           "corner_tl": (ys < bh) & (xs < bw), "corner_tr": (ys < bh) & (xs >= W - bw),
           "corner_bl": (ys >= H - bh) & (xs < bw), "corner_br": (ys >= H - bh) & (xs >= W - bw)}
    return out


PATTERN_NAMES = ["empty", "full", "checker", "hole", "diag", "top", "bottom", "left", "right", "corner_tl", "corner_tr",
                 "corner_bl", "corner_br"]


def level_frames(n, H, W):
    """fp32 [n, 3, H, W]: every channel holds fp32((p / 255 - mean_c) / std_c) for p = 0..255, then -5 and +5,
    cycling over the pixels (H W >= 258 holds them all)"""
    p = np.arange(H * W) % 258
    out = np.empty((n, 3, H, W), np.float32)
    for c in range(3):
        v = ((np.minimum(p, 255) / 255.0 - MEAN[c]) / STD[c]).astype(np.float32)
        v[p == 256], v[p == 257] = -5.0, 5.0
        for f in range(n):
            out[f, c] = np.roll(v, 37 * f + 11 * c).reshape(H, W)
    return out


def _masks(rng, stored, C, H, W, shift, kind):
    """[stored, C, H, W]: category c of stored frame f is pattern (c + f + shift); two neighbouring categories
    therefore overlap (full / checker / hole ...).  uint8 of 0 / 1 (and some 255), or fp32 logits at +-3 with the
    special values sprinkled in"""
    pats = patterns(H, W)
    m = np.stack([np.stack([pats[PATTERN_NAMES[(c + f + shift) % len(PATTERN_NAMES)]] for c in range(C)])
                  for f in range(stored)])
    if kind == "u8":
        out = m.astype(np.uint8)
        out[m & (rng.random(m.shape) < 0.1)] = 255
        return out
    out = np.where(m, 3.0, -3.0).astype(np.float32)
    sel = rng.random(m.shape) < 0.25
    out[sel] = SPECIAL_LOGITS[rng.integers(0, len(SPECIAL_LOGITS), int(sel.sum()))]
    return out


def marker_sets(H, W, palette):
    C = len(palette)

    def col(i):
        return [int(v) for v in palette[i % C]]
    cx, cy = W // 2, H // 2
    sets = {"none": [],
            "overlapping": [[DISC, cx, cy] + [0, 0] + col(0), [CROSS, cx + 3, cy + 2, 0, 0] + col(1),
                            [BOX, cx - 6, cy - 5, cx + 7, cy + 6] + col(2), [DISC, cx + 5, cy, 0, 0] + col(3),
                            [BOX, 0, 0, W - 1, H - 1] + col(4)],
            "outside": [[DISC, -3, 2, 0, 0] + col(0), [CROSS, W + 2, H - 1, 0, 0] + col(1),
                        [DISC, W + 40, -50, 0, 0] + col(2), [CROSS, -30, H + 30, 0, 0] + col(3),
                        [BOX, -4, -4, 3, 2] + col(4), [BOX, W + 5, H + 5, W + 9, H + 9] + col(5),
                        [DISC, 2 ** 31 - 1, -2 ** 31, 0, 0] + col(6), [BOX, -2 ** 31, -2 ** 31, 2 ** 31 - 1, 2 ** 31 - 1] + col(7)],
            "boxes": [[BOX, cx + 2, cy, cx - 2, cy + 4] + col(0), [BOX, cx, cy + 3, cx + 4, cy - 3] + col(1),  # inverted
                      [BOX, cx, cy, cx, cy] + col(2), [BOX, 0, 0, min(W - 1, 2), min(H - 1, 3)] + col(3),  # one pixel, thin
                      [9, cx, cy, 0, 0] + col(4)]}  # an unknown kind paints nothing
    rng = np.random.default_rng(256)
    many = []
    for i in range(256):
        k = int(rng.integers(0, 3))
        x, y = int(rng.integers(-5, W + 5)), int(rng.integers(-5, H + 5))
        many.append([k, x, y, x + int(rng.integers(-2, 12)), y + int(rng.integers(-2, 12))] + col(i))
    sets["many"] = many
    return {k: np.asarray(v, np.int32).reshape(-1, 8) for k, v in sets.items()}


def make_case(name, n, C, H, W, img="f32", gt="u8", pred="f32", step=1, markers="none", prompt=None, levels=False,
              seed=0):
    rng = np.random.default_rng(seed)
    stored = (n - 1) * step + 1
    if img == "u8":
        frames = rng.integers(0, 256, (stored, H, W, 3), dtype=np.uint8)
        frame0 = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    else:
        frames = level_frames(stored, H, W) if levels else (rng.standard_normal((stored, 3, H, W)) * 1.3).astype(np.float32)
        frame0 = (rng.standard_normal((3, H, W)) * 1.3).astype(np.float32)
    pal = palette_of(C)
    return {"name": name, "n": n, "C": C, "H": H, "W": W, "step": step, "frames": frames, "frame0": frame0,
            "gt": _masks(rng, stored, C, H, W, 0, gt), "pred": _masks(rng, stored, C, H, W, 4, pred),
            "prompt": None if prompt is None else _masks(rng, 1, C, H, W, 7, prompt)[0],
            "markers": marker_sets(H, W, pal)[markers], "palette": pal}


def make_cases():
    cases = []
    for i, (H, W) in enumerate(SIZES):
        s = f"{H}x{W}"
        cases += [make_case(f"{s}-n1-C1", 1, 1, H, W, seed=10 * i),
                  make_case(f"{s}-n3-C13-overlapping", 3, 13, H, W, markers="overlapping", seed=10 * i + 1),
                  make_case(f"{s}-n1-C64-u8img-swapped", 1, 64, H, W, img="u8", gt="f32", pred="u8", markers="outside",
                            seed=10 * i + 2),
                  make_case(f"{s}-n3-C13-stride2", 3, 13, H, W, step=2, markers="boxes", seed=10 * i + 3),
                  make_case(f"{s}-n1-C13-maskprompt", 1, 13, H, W, prompt="f32", seed=10 * i + 4)]
    cases += [make_case("17x33-n3-C64-levels", 3, 64, 17, 33, levels=True, markers="many", seed=91),
              make_case("64x64-n3-C13-u8img-stride2", 3, 13, 64, 64, img="u8", step=2, gt="u8", pred="u8",
                        prompt="u8", seed=92),
              make_case("130x66-n3-C64-many", 3, 64, 130, 66, markers="many", seed=93),
              make_case("5x7-n3-C1-full", 3, 1, 5, 7, markers="many", seed=94)]
    return cases


MID_CASE = "64x64-n3-C13-u8img-stride2"  # the one replayed from a captured graph


def case_bytes(c):
    """the case in the input format of csrc/viz_host_check.cpp"""
    def kind(a):
        return int(a.dtype == np.float32)
    hdr = [c["n"], c["C"], c["H"], c["W"], int(c["frames"].dtype == np.uint8), kind(c["gt"]), kind(c["pred"]),
           -1 if c["prompt"] is None else kind(c["prompt"]), len(c["markers"]), c["step"]]
    parts = [np.asarray(hdr, np.int32), c["frames"], c["frame0"], c["gt"], c["pred"]]
    if c["prompt"] is not None:
        parts.append(c["prompt"])
    parts += [c["palette"], c["markers"]]
    return b"".join(np.ascontiguousarray(p).tobytes() for p in parts)


# ------------------------------------------------------------------------------------------------ the public function
def clip(T, C, H, W, T_pred, kind, seed=0):
    """frames, ground truth, outs_per_frame and obj_to_cat of a synthetic clip with point / box / mask prompts
    (host tensors, the arguments of create_visualization_gif)"""
    import torch
    rng = np.random.default_rng(seed)
    frames = torch.from_numpy((rng.standard_normal((T, 3, H, W)) * 1.3).astype(np.float32))
    gt = torch.from_numpy(_masks(rng, T, C, H, W, 0, "u8") > 0)
    preds = torch.from_numpy(_masks(rng, T_pred, C, H, W, 3, "f32"))
    obj_to_cat = [0, C - 1, C // 2, 0]
    O = len(obj_to_cat)
    point_inputs = mask_inputs = None
    if kind == "point":
        coords = torch.from_numpy(rng.uniform(-4, max(H, W) + 4, (O, 3, 2)).astype(np.float32))
        labels = torch.tensor([[1, 0, -1], [1, 1, 0], [0, -1, -1], [1, 0, 1]], dtype=torch.int32)
        point_inputs = {"point_coords": coords, "point_labels": labels}
    elif kind == "box":
        lo = rng.uniform(0, W / 2, (O, 1, 2))
        coords = torch.from_numpy(np.concatenate([lo, lo + rng.uniform(-1, W / 2, (O, 1, 2))], 1).astype(np.float32))
        point_inputs = {"point_coords": coords, "point_labels": torch.tensor([[2, 3]] * O, dtype=torch.int32)}
    else:
        mask_inputs = torch.from_numpy((rng.random((O, H, W)) < 0.3).astype(np.float32))
    outs = [{"multistep_pred_multimasks_high_res": [preds[t].reshape(C, 1, H, W)], "point_inputs": None,
             "mask_inputs": None} for t in range(T_pred)]
    outs[0]["point_inputs"], outs[0]["mask_inputs"] = point_inputs, mask_inputs
    return frames, gt, outs, obj_to_cat


def model_of_clip(frames, gt, outs, obj_to_cat, max_length, stride):
    """the model on the reference's selection: length = min(max_length, T_frames, T_preds), range(0, length, stride)"""
    idx = list(range(0, min(max_length, frames.shape[0], len(outs)), stride))
    C = gt.shape[1]
    pal = palette_of(C)
    pred = np.stack([outs[i]["multistep_pred_multimasks_high_res"][0].cpu().numpy().reshape(gt.shape[1:]) for i in idx])
    markers = prompt = None
    if outs[0]["point_inputs"] is not None:
        p = outs[0]["point_inputs"]
        markers = markers_from_points(p["point_coords"].cpu().numpy(), p["point_labels"].cpu().numpy(), obj_to_cat, pal)
    else:
        m = outs[0]["mask_inputs"].cpu().numpy()
        prompt = np.zeros(tuple(gt.shape[1:]), np.float32)
        for o, cat in enumerate(obj_to_cat):
            prompt[cat] = np.maximum(prompt[cat], m[o].reshape(gt.shape[2:]))
    f = frames.cpu().numpy()
    out = composites(f[idx], f[0], gt.cpu().numpy()[idx], pred, pal, markers, prompt)
    return out.transpose(0, 3, 1, 2)


# ------------------------------------------------------------------------------------------------ the viewer
def build_viewer_tree(root):
    """a tiny evaluation run on disk: PNG frames of two videos (20 x 28 and 9 x 13), a COCO file with category ids
    0, 1 and 3, a predict.json and a prompt.pkl (points on vidA's second frame, a box and then masks on vidB).
    -> {clip name: (frames uint8 [n, H, W, 3], prompt frame, gt [n, 4, H, W], pred, markers or None, prompt mask
    or None)}: what the composites are made of, for the model"""
    import json
    import os
    import pickle

    from PIL import Image

    from sam2_video.data import rle
    from sam2_video.eval.utils import ClipRange, PromptInfo, PromptObj
    rng = np.random.default_rng(77)
    os.makedirs(os.path.join(root, "img"), exist_ok=True)
    cats, C = [0, 1, 3], 4
    pal = palette_of(C)
    images, anns, preds, want, prompts = [], [], [], {}, []
    iid = 0
    for vid, (H, W), n in (("vidA", (20, 28), 3), ("vidB", (9, 13), 2)):
        pats = patterns(H, W)
        frames = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
        gt, pr = np.zeros((n, C, H, W), np.uint8), np.zeros((n, C, H, W), np.uint8)
        for f in range(n):
            name = os.path.join("img", f"{vid}_{f:03d}.png")
            Image.fromarray(frames[f]).save(os.path.join(root, name))
            images.append({"id": iid, "file_name": name, "path": name, "height": H, "width": W, "video_id": vid,
                           "order_in_video": f})
            for k, c in enumerate(cats):
                g = pats[PATTERN_NAMES[(2 + f + 3 * k) % len(PATTERN_NAMES)]]
                p = pats[PATTERN_NAMES[(5 + f + 2 * k) % len(PATTERN_NAMES)]]
                for src, dst, lst in ((g, gt, anns), (p, pr, preds)):
                    if src.any():
                        dst[f, c] |= src
                        lst.append({"id": len(lst), "image_id": iid, "category_id": c, "segmentation": rle.encode(src),
                                    "iscrowd": 0, "bbox": [0, 0, W, H], "area": int(src.sum()), "score": 0.5})
            if f == 0 and vid == "vidA":  # two annotations of one category are OR-ed
                extra = pats["corner_br"]
                gt[f, 1] |= extra
                anns.append({"id": len(anns), "image_id": iid, "category_id": 1, "segmentation": rle.encode(extra),
                             "iscrowd": 0, "bbox": [0, 0, W, H], "area": int(extra.sum())})
            iid += 1
        if vid == "vidA":
            objs = [PromptObj(mask=None, bbox=None, points=[[5.7, 6.2], [20.1, 11.9]], obj_id=1, pos_or_neg_label=[1, 0]),
                    PromptObj(mask=None, bbox=None, points=[[26.0, 18.5]], obj_id=3 + C, pos_or_neg_label=[1])]
            prompts.append(PromptInfo(objs, 1, "point", vid, "", ClipRange(0, 2)))
            mk = np.asarray([[DISC, 5, 6, 0, 0] + pal[1].tolist(), [CROSS, 20, 11, 0, 0] + pal[1].tolist(),
                             [DISC, 26, 18, 0, 0] + pal[3].tolist()], np.int32)
            want["vidA_0"] = (frames, frames[1], gt, pr, mk, None)
        else:
            objs = [PromptObj(mask=None, bbox=[1.5, 2.0, 9.9, 7.2], points=None, obj_id=0, pos_or_neg_label=None)]
            prompts.append(PromptInfo(objs, 0, "box", vid, "", ClipRange(0, 1)))
            want["vidB_0"] = (frames, frames[0], gt, pr, np.asarray([[BOX, 1, 2, 9, 7] + pal[0].tolist()], np.int32), None)
            m0, m1 = pats["left"].astype(np.uint8), pats["checker"].astype(np.uint8)
            objs = [PromptObj(mask=m0, bbox=None, points=None, obj_id=3, pos_or_neg_label=None),
                    PromptObj(mask=m1, bbox=None, points=None, obj_id=3 + C, pos_or_neg_label=None),
                    PromptObj(mask=m1, bbox=None, points=None, obj_id=0, pos_or_neg_label=None)]
            prompts.append(PromptInfo(objs, 1, "mask", vid, "", ClipRange(1, 1)))
            pm = np.zeros((C, H, W), np.uint8)
            pm[3], pm[0] = m0 | m1, m1
            want["vidB_1"] = (frames[1:], frames[1], gt[1:], pr[1:], None, pm)
    with open(os.path.join(root, "gt.json"), "w") as f:
        json.dump({"images": images, "annotations": anns, "categories": [{"id": c, "name": f"c{c}"} for c in cats]}, f)
    with open(os.path.join(root, "predict.json"), "w") as f:
        json.dump(preds, f)
    with open(os.path.join(root, "prompt.pkl"), "wb") as f:
        pickle.dump(prompts, f)
    return want


def viewer_model(parts):
    frames, frame0, gt, pred, markers, prompt = parts
    return composites(frames, frame0, gt, pred, palette_of(gt.shape[1]), markers, prompt).transpose(0, 3, 1, 2)


def read_png_series(out_dir, name):
    """[n, 3, H, W] of <out_dir>/<name>_f{i}.png"""
    import os

    from PIL import Image
    files = sorted((f for f in os.listdir(out_dir) if f.startswith(name + "_f") and f.endswith(".png")),
                   key=lambda f: int(f[len(name) + 2:-4]))
    return np.stack([np.asarray(Image.open(os.path.join(out_dir, f)).convert("RGB")) for f in files]).transpose(0, 3, 1, 2)
