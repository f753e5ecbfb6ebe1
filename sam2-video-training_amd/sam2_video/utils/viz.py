"""Training visualisation (reference sam2_video/utils/viz.py): 2 x 2 composite frames built on the device and
written as GIF / PNG with Pillow.

The reference copies the [T, C, H, W] fp32 logits, the frames and the ground truth to the host, draws with cv2 and
matplotlib and hands the figure to wandb.Video; its colours come from an unseeded random.random().  Here the
picture is defined exactly, in integers (csrc/viz_pixel.h), composed by two HIP launches
(kernels.ops.viz_pack / viz_compose) from tensors that are already on the device, and only the finished uint8
composites cross the bus.  `on_device=False` computes the same bytes in numpy.

Composite of selected frame i, uint8 [2H, 2W, 3], no text (the reference's 2 x 2 order):
    frame i                | frame i + ground-truth overlay
    frame 0 + prompts      | frame i + prediction overlay
Category c is set at a pixel where its value is > 0.5.  This is the reference's rule for BOTH sides
(`mask_array[c] > 0.5`): it is applied to the ground truth and to the raw prediction logits alike, i.e. the
prediction panel shows logit > 0.5, not probability > 0.5.  It is kept as it is.
"""
from __future__ import annotations

import colorsys
import os
import warnings
from typing import Any, Dict, List, Optional, Sequence

import numpy as np
import torch

MAX_MARKERS = 256
DISC, CROSS, BOX = 0, 1, 2
_MEAN = np.array([0.485, 0.456, 0.406])
_STD = np.array([0.229, 0.224, 0.225])


def category_palette(num_categories: int) -> np.ndarray:
    """uint8 [C, 3]: colors[c] = int(255 * hsv_to_rgb(c / C, 0.9, 0.9)).  The reference's hues with fixed
    saturation and value (it draws both at random in [0.8, 1] on every call)."""
    C = int(num_categories)
    return np.array([[int(255 * v) for v in colorsys.hsv_to_rgb(c / C, 0.9, 0.9)] for c in range(C)],
                    dtype=np.uint8).reshape(C, 3)


def prompt_type_of(point_inputs) -> str:
    """viz.py:270-277: box when a label 2 or 3 occurs, point otherwise, mask without point inputs"""
    if point_inputs is None:
        return "mask"
    labels = np.asarray(torch.as_tensor(point_inputs["point_labels"]).cpu())
    return "bbox" if bool(((labels == 2) | (labels == 3)).any()) else "point"


def prompt_markers(point_inputs, obj_to_cat: Sequence[int], palette: np.ndarray) -> np.ndarray:
    """The marker table int32 [M, 8] = {kind, x1, y1, x2, y2, r, g, b} of frame 0's point inputs (viz.py:155-210),
    object o in colors[obj_to_cat[o]], coordinates truncated by int() as the reference does.  Point prompts: a
    disc per label-1 point, a cross per label-0 point (other labels, the padding's -1, draw nothing).  Box prompts:
    one box per object from its last label-2 (x1, y1) and label-3 (x2, y2) points, 0 where one is absent.  At
    most 256 markers: further ones are dropped with a warning."""
    coords = np.asarray(torch.as_tensor(point_inputs["point_coords"]).detach().cpu(), dtype=np.float64)
    labels = np.asarray(torch.as_tensor(point_inputs["point_labels"]).detach().cpu())
    kind = prompt_type_of(point_inputs)
    rows = []
    for o in range(labels.shape[0]):
        r, g, b = (int(v) for v in palette[obj_to_cat[o]])
        if kind == "bbox":
            x1 = y1 = x2 = y2 = 0
            for p in range(labels.shape[1]):
                if labels[o, p] == 2:
                    x1, y1 = int(coords[o, p, 0]), int(coords[o, p, 1])
                if labels[o, p] == 3:
                    x2, y2 = int(coords[o, p, 0]), int(coords[o, p, 1])
            rows.append([BOX, x1, y1, x2, y2, r, g, b])
            continue
        for p in range(labels.shape[1]):
            if labels[o, p] in (0, 1):
                rows.append([DISC if labels[o, p] == 1 else CROSS, int(coords[o, p, 0]), int(coords[o, p, 1]), 0, 0,
                             r, g, b])
    if len(rows) > MAX_MARKERS:
        warnings.warn(f"visualisation: {len(rows)} prompt markers, the first {MAX_MARKERS} are drawn", UserWarning,
                      stacklevel=2)
        rows = rows[:MAX_MARKERS]
    return np.asarray(rows, dtype=np.int32).reshape(-1, 8)


# ------------------------------------------------------------------------------------------------ numpy path
def frames_to_u8(frames: np.ndarray) -> np.ndarray:
    """[n, 3, H, W] normalised fp32 -> uint8 [n, H, W, 3] (viz.py:46-54, float64 as numpy promotes it); uint8
    [n, H, W, 3] passes through"""
    if frames.dtype == np.uint8:
        return frames
    v = frames.astype(np.float64).transpose(0, 2, 3, 1) * _STD + _MEAN
    v = np.where(v > 0, np.minimum(v, 1.0), 0.0)
    return (v * 255).astype(np.uint8)


def pack_words_host(masks: np.ndarray) -> np.ndarray:
    """[n, C, H, W] -> uint64 [n, H, W], bit c = masks[:, c] > 0.5"""
    n, C, H, W = masks.shape
    words = np.zeros((n, H, W), np.uint64)
    for c in range(C):
        words |= (masks[:, c] > 0.5).astype(np.uint64) << np.uint64(c)
    return words


def _top_colour(words: np.ndarray, palette: np.ndarray) -> np.ndarray:
    """[.., 3] colour of the highest set bit, 0 where none is set"""
    out = np.zeros(words.shape + (3,), np.uint8)
    for c in range(palette.shape[0]):
        out[(words >> np.uint64(c)) & np.uint64(1) == 1] = palette[c]
    return out


def overlay_panel_host(base: np.ndarray, words: np.ndarray, palette: np.ndarray) -> np.ndarray:
    """base uint8 [H, W, 3], words uint64 [H, W] -> the blended panel with its contour band"""
    H, W = words.shape
    over = _top_colour(words, palette).astype(np.int32)
    out = ((4 * base.astype(np.int32) + over + 2) // 5).astype(np.uint8)
    full = np.uint64(0xFFFFFFFFFFFFFFFF)
    pad_any = np.zeros((H + 2, W + 2), np.uint64)
    pad_all = np.full((H + 2, W + 2), full, np.uint64)
    pad_any[1:-1, 1:-1] = words
    pad_all[1:-1, 1:-1] = words
    any_, all_ = np.zeros((H, W), np.uint64), np.full((H, W), full, np.uint64)
    for dy in range(3):
        for dx in range(3):
            any_ |= pad_any[dy:dy + H, dx:dx + W]
            all_ &= pad_all[dy:dy + H, dx:dx + W]
    band = any_ & ~all_
    on = band != 0
    out[on] = _top_colour(band, palette)[on]
    return out


def draw_markers_host(img: np.ndarray, markers: np.ndarray) -> np.ndarray:
    """img uint8 [H, W, 3] (changed in place), markers int32 [M, 8] in table order"""
    H, W = img.shape[:2]
    ys, xs = np.mgrid[0:H, 0:W].astype(np.int64)
    for kind, x1, y1, x2, y2, r, g, b in markers.astype(np.int64):
        dx, dy = xs - x1, ys - y1
        if kind == BOX:
            ex, ey = x2 - xs, y2 - ys
            inside = (dx >= 0) & (dy >= 0) & (ex >= 0) & (ey >= 0)
            img[inside & (np.minimum(np.minimum(dx, ex), np.minimum(dy, ey)) < 2)] = (r, g, b)
        elif kind == DISC:
            cx, cy = np.clip(dx, -10, 10), np.clip(dy, -10, 10)  # (far pixels stay far; no overflow in the squares)
            d2 = cx * cx + cy * cy
            img[d2 < 49] = (r, g, b)
            img[(d2 >= 49) & (d2 <= 81)] = (255, 255, 255)
        elif kind == CROSS:
            ax, ay = np.abs(dx), np.abs(dy)
            img[((ax <= 1) & (ay <= 8)) | ((ay <= 1) & (ax <= 8))] = (r, g, b)
    return img


def compose_host(frames_u8, frame0_u8, gt_words, pred_words, palette, markers=None, prompt_words=None) -> np.ndarray:
    """the composites uint8 [n, 2H, 2W, 3] in numpy (the bytes of kernels.ops.viz_compose)"""
    n, H, W = gt_words.shape
    out = np.empty((n, 2 * H, 2 * W, 3), np.uint8)
    if prompt_words is not None:
        prompt = overlay_panel_host(frame0_u8, prompt_words, palette)
    else:
        prompt = frame0_u8.copy()
        if markers is not None and len(markers):
            draw_markers_host(prompt, markers)
    for f in range(n):
        out[f, :H, :W] = frames_u8[f]
        out[f, :H, W:] = overlay_panel_host(frames_u8[f], gt_words[f], palette)
        out[f, H:, :W] = prompt
        out[f, H:, W:] = overlay_panel_host(frames_u8[f], pred_words[f], palette)
    return out


# ------------------------------------------------------------------------------------------------ public surface
_STAGING: Dict[Any, torch.Tensor] = {}


def _pinned(nbytes: int) -> torch.Tensor:
    """one pinned staging buffer for the copy back, grown when a larger picture comes"""
    buf = _STAGING.get("buf")
    if buf is None or buf.numel() < nbytes:
        buf = _STAGING["buf"] = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
    return buf[:nbytes]


def _category_masks_of_objects(mask_inputs, obj_to_cat, C):
    """viz.py:212-219: prompt_mask[cat] = max over that category's objects -> bool [1, C, H, W]"""
    m = mask_inputs.detach()
    m = m.reshape(m.shape[0], *m.shape[-2:]) > 0.5  # (max then > 0.5 == any of > 0.5)
    out = torch.zeros(1, C, *m.shape[-2:], dtype=torch.bool, device=m.device)
    for cat in sorted(set(int(c) for c in obj_to_cat)):
        out[0, cat] = m[[o for o, c in enumerate(obj_to_cat) if int(c) == cat]].any(dim=0)
    return out


def create_visualization_gif(frames: torch.Tensor, gt_masks: torch.Tensor, outs_per_frame: List[Dict[str, Any]],
                             obj_to_cat: List[int], max_length: int = 4, stride: int = 1, *, on_device: bool = True,
                             to_host: bool = False):
    """The reference's call (viz.py:249-310) and its frame selection: length = min(max_length, T_frames, T_preds),
    indices = range(0, length, stride); prompt type from frame 0's labels.  Returns uint8 [N, 3, 2H, 2W], the
    reference's `gif_np` layout.

    frames [T, 3, H, W] fp32 ImageNet-normalised (batch.img_batch.squeeze(1)) or uint8 [T, H, W, 3]; gt_masks
    [T, C, H, W] bool / uint8 / fp32; outs_per_frame[t]["multistep_pred_multimasks_high_res"][0] the category-level
    logits [C, 1, H, W] (or [C, H, W]); outs_per_frame[0]["point_inputs"] / ["mask_inputs"] the prompts.

    on_device=True: two HIP launches on the current stream; the result is a device tensor, or with to_host=True a
    numpy view of the module's pinned staging buffer (one synchronising copy; the next call overwrites it).
    on_device=False: the same bytes from numpy, returned as a numpy array."""
    preds = [o["multistep_pred_multimasks_high_res"][0] for o in outs_per_frame]
    length = min(int(max_length), int(frames.shape[0]), len(preds))
    idx = list(range(0, length, int(stride)))
    u8 = frames.dtype == torch.uint8
    H, W = (frames.shape[1], frames.shape[2]) if u8 else (frames.shape[2], frames.shape[3])
    if not idx:
        empty = torch.empty(0, 3, 2 * H, 2 * W, dtype=torch.uint8, device=frames.device if on_device else "cpu")
        return empty if on_device and not to_host else empty.cpu().numpy()
    C = int(gt_masks.shape[1])
    palette = category_palette(C)
    point_inputs = outs_per_frame[0].get("point_inputs")
    markers = prompt_mask = None
    if point_inputs is not None:
        markers = prompt_markers(point_inputs, obj_to_cat, palette)
    else:
        mask_inputs = outs_per_frame[0]["mask_inputs"]
        if tuple(mask_inputs.shape[-2:]) != (H, W):
            raise ValueError(f"mask prompts of size {tuple(mask_inputs.shape[-2:])} on frames of size {(H, W)}")
        prompt_mask = _category_masks_of_objects(mask_inputs, obj_to_cat, C)
    sel_frames = frames.detach()[0:length:int(stride)]
    sel_gt = gt_masks.detach()[0:length:int(stride)]
    if sel_gt.dtype not in (torch.bool, torch.uint8, torch.float32):
        sel_gt = sel_gt > 0.5
    sel_pred = torch.stack([preds[i].detach().reshape(C, H, W) for i in idx])  # the one gathering copy
    if sel_pred.dtype != torch.float32:
        sel_pred = sel_pred.float()
    if not on_device:
        fu8 = frames_to_u8(sel_frames.cpu().numpy())
        f0 = frames_to_u8(frames.detach()[0:1].cpu().numpy())[0]
        pw = None if prompt_mask is None else pack_words_host(prompt_mask.cpu().numpy())[0]
        out = compose_host(fu8, f0, pack_words_host(sel_gt.cpu().numpy()), pack_words_host(sel_pred.cpu().numpy()),
                           palette, markers, pw)
        return np.ascontiguousarray(out.transpose(0, 3, 1, 2))
    from ..kernels import ops
    dev = frames.device
    if sel_frames.shape[0] > 1 and not sel_frames[0].is_contiguous():
        sel_frames = sel_frames.contiguous()
    frame0 = frames.detach()[0].contiguous()
    pal = torch.from_numpy(palette).to(dev)
    mk = torch.from_numpy(markers).to(dev) if markers is not None and len(markers) else None
    pw = None if prompt_mask is None else ops.viz_pack(prompt_mask.to(dev))[0]
    out = ops.viz_compose(sel_frames, frame0, ops.viz_pack(sel_gt.to(dev)), ops.viz_pack(sel_pred.to(dev)), pal, mk, pw)
    if not to_host:
        return out.permute(0, 3, 1, 2)
    host = _pinned(out.numel()).view(out.shape)
    host.copy_(out, non_blocking=True)
    torch.cuda.current_stream(dev).synchronize()
    return host.numpy().transpose(0, 3, 1, 2)


def save_visualization(array, path, fps: int = 4, caption: Optional[str] = None, format: str = "gif") -> List[str]:
    """uint8 [N, 3, H, W] (numpy or tensor) -> an animated GIF at `path` (Pillow: save_all, duration = 1000 / fps
    ms per frame, loop = 0 = forever, `caption` as the GIF comment), or with format="png" one lossless PNG per
    frame, `<path without extension>_f{i}.png` -- GIF quantises every frame to 256 colours, PNG keeps the exact
    bytes.  Returns the paths written."""
    from PIL import Image
    a = array.detach().cpu().numpy() if torch.is_tensor(array) else np.asarray(array)
    if a.dtype != np.uint8 or a.ndim != 4 or a.shape[1] != 3:
        raise ValueError(f"save_visualization: uint8 [N, 3, H, W] expected, got {a.dtype} {a.shape}")
    if a.shape[0] == 0:
        return []
    imgs = [Image.fromarray(np.ascontiguousarray(f.transpose(1, 2, 0))) for f in a]  # (uint8 [H, W, 3] = RGB)
    path = str(path)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    fmt = str(format).lower()
    if fmt == "png":
        root = os.path.splitext(path)[0]
        out = [f"{root}_f{i}.png" for i in range(len(imgs))]
        for im, p in zip(imgs, out):
            im.save(p, format="PNG")
        return out
    if fmt != "gif":
        raise ValueError(f"save_visualization: format {format!r} (gif or png)")
    kw = {"comment": caption} if caption else {}
    imgs[0].save(path, format="GIF", save_all=True, append_images=imgs[1:], duration=1000 / fps, loop=0, **kw)
    return [path]
