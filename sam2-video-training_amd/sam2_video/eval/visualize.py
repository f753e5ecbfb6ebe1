"""Post-hoc viewer (the role of the reference's scripts/visualize_cv.py): ground truth, prediction and prompts of
an evaluation run as the 2 x 2 composites of utils/viz.py, one GIF (or PNG series) per clip.

    python -m sam2_video.eval.visualize --gt COCO.json --predict predict.json [--prompt prompt.pkl] --out DIR
                                        [--format gif|png] [--image-root DIR] [--max-frames N] [--fps 4] [--host]

Per clip the frames are decoded to uint8 RGB with Pillow and uploaded; the ground-truth and predicted RLE
annotations become per-category masks on the device through the existing RLE entry s2h_rle_catmasks
(ops.rle_catmasks with identity row / column maps: only the run boundaries are uploaded, annotations of one
category are OR-ed); the compositor then runs with its uint8 image kind (ops.viz_pack / ops.viz_compose), in chunks
of frames.  `--host` decodes with data/rle.py and composes in numpy: the same bytes.

Category c is drawn in colors[c] of a palette of max(category id) + 1 entries (the evaluation's `mod`; at most
64).  With --prompt a clip is a PromptInfo of prompt.pkl (its clip_range of its video, the prompts drawn on its
prompt frame: points as discs / crosses, boxes as rectangles, masks as an overlay; object obj_id has category
obj_id % mod); without it a clip is a whole video and the prompt panel shows its first frame unmarked.  Files:
<out>/<video_id>_<first order_in_video>.gif (or _f{i}.png)."""
from __future__ import annotations

import argparse
import json
import os
import pickle
from typing import Dict, List, Optional

import numpy as np
import torch

from ..data import rle
from ..utils import viz as V
from .utils import sort_dicts_by_field

CHUNK = 8  # frames composed per launch (n * 2H * 2W * 3 < 2^31 and a bounded device footprint)


def _frame_rgb(image: Dict, image_root: Optional[str]) -> np.ndarray:
    from PIL import Image
    path = image.get("path") or image["file_name"]
    if image_root and not os.path.isabs(path):
        path = os.path.join(image_root, path)
    with Image.open(path) as im:
        return np.asarray(im.convert("RGB"), dtype=np.uint8)


def _masks_host(frames: List[Dict], anns: Dict[int, List[Dict]], C: int, H: int, W: int) -> np.ndarray:
    out = np.zeros((len(frames), C, H, W), np.uint8)
    for f, image in enumerate(frames):
        for a in anns.get(int(image["id"]), []):
            c = int(a["category_id"])
            if 0 <= c < C:
                out[f, c] |= rle.decode(a["segmentation"])
    return out


def _masks_device(frames, anns, C, H, W, device):
    from ..kernels import ops
    counts, cats, frame_off = [], [], [0]
    for image in frames:
        for a in anns.get(int(image["id"]), []):
            h, w, cnts = rle.counts_of(a["segmentation"])
            if (h, w) != (H, W):
                raise ValueError(f"annotation of image {image['id']}: mask {(h, w)}, image {(H, W)}")
            counts.append(cnts)
            cats.append(int(a["category_id"]))
        frame_off.append(len(counts))
    run_off, run_end = ops.rle_runs(counts, H, W)

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(device)
    return ops.rle_catmasks(up(run_off), up(run_end), up(cats), up(frame_off), H, W, up(np.arange(H)), up(np.arange(W)), C)


def _prompt_of(info, C: int, H: int, W: int, palette: np.ndarray, mod: int):
    """(marker table or None, prompt mask [C, H, W] or None) of a PromptInfo"""
    if info is None:
        return None, None
    kind = str(info.prompt_type).lower()
    if kind == "mask":
        pm = np.zeros((C, H, W), np.uint8)
        for o in info.prompt_objs:
            pm[o.obj_id % mod] |= (np.asarray(o.mask).reshape(H, W) > 0.5).astype(np.uint8)
        return None, pm
    rows = []
    for o in info.prompt_objs:
        col = [int(v) for v in palette[o.obj_id % mod]]
        if kind in ("box", "bbox"):
            rows.append([V.BOX] + [int(v) for v in o.bbox[:4]] + col)
        else:
            for (x, y), lab in zip(o.points, o.pos_or_neg_label):
                if lab in (0, 1):
                    rows.append([V.DISC if lab == 1 else V.CROSS, int(x), int(y), 0, 0] + col)
    return np.asarray(rows[:V.MAX_MARKERS], np.int32).reshape(-1, 8), None


def render_clip(frames: List[Dict], gt: Dict[int, List[Dict]], pred: Dict[int, List[Dict]], C: int, info=None,
                image_root: Optional[str] = None, on_device: bool = True, device="cuda") -> np.ndarray:
    """the composites uint8 [n, 3, 2H, 2W] of one clip (frames in order); the prompt panel shows the prompt
    frame of `info`, or the first frame"""
    H, W = int(frames[0]["height"]), int(frames[0]["width"])
    palette = V.category_palette(C)
    imgs = np.stack([_frame_rgb(im, image_root) for im in frames])
    if imgs.shape[1:3] != (H, W):
        raise ValueError(f"{frames[0].get('file_name')}: decoded {imgs.shape[1:3]}, COCO says {(H, W)}")
    first = 0
    if info is not None:
        first = next((k for k, im in enumerate(frames) if int(im["order_in_video"]) == int(info.frame_idx)), 0)
    markers, pmask = _prompt_of(info, C, H, W, palette, C)
    out = []
    for a in range(0, len(frames), CHUNK):
        part = frames[a:a + CHUNK]
        if not on_device:
            pw = None if pmask is None else V.pack_words_host(pmask[None])[0]
            out.append(V.compose_host(imgs[a:a + CHUNK], imgs[first], V.pack_words_host(_masks_host(part, gt, C, H, W)),
                                      V.pack_words_host(_masks_host(part, pred, C, H, W)), palette, markers, pw))
            continue
        from ..kernels import ops
        dev = torch.device(device)
        pw = None if pmask is None else ops.viz_pack(torch.from_numpy(pmask[None]).to(dev))[0]
        mk = torch.from_numpy(markers).to(dev) if markers is not None and len(markers) else None
        comp = ops.viz_compose(torch.from_numpy(imgs[a:a + CHUNK]).to(dev), torch.from_numpy(imgs[first]).to(dev),
                               ops.viz_pack(_masks_device(part, gt, C, H, W, dev)),
                               ops.viz_pack(_masks_device(part, pred, C, H, W, dev)),
                               torch.from_numpy(palette).to(dev), mk, pw)
        out.append(comp.cpu().numpy())
    return np.concatenate(out).transpose(0, 3, 1, 2)


def _by_image(anns: List[Dict]) -> Dict[int, List[Dict]]:
    out: Dict[int, List[Dict]] = {}
    for a in anns:
        out.setdefault(int(a["image_id"]), []).append(a)
    return out


def visualize(gt_path, predict_path, out_dir, prompt_path=None, format="gif", image_root=None, max_frames=None, fps=4,
              on_device=True) -> List[str]:
    """-> the files written"""
    with open(gt_path) as f:
        coco = json.load(f)
    with open(predict_path) as f:
        predict = json.load(f)
    predict = predict["annotations"] if isinstance(predict, dict) else predict
    C = max(int(c["id"]) for c in coco["categories"]) + 1
    if C > 64:
        raise ValueError(f"category ids up to {C - 1}: the compositor holds 64 categories")
    gt, pred = _by_image(coco["annotations"]), _by_image(predict)
    videos: Dict[str, List[Dict]] = {}
    for im in coco["images"]:
        videos.setdefault(im["video_id"], []).append(im)
    clips = []
    if prompt_path:
        with open(prompt_path, "rb") as f:
            for info in pickle.load(f):
                fr = [im for im in videos.get(info.video_id, [])
                      if info.clip_range.start_idx <= int(im["order_in_video"]) <= info.clip_range.end_idx]
                clips.append((info.video_id, fr, info))
    else:
        clips = [(vid, fr, None) for vid, fr in videos.items()]
    written = []
    for vid, fr, info in clips:
        fr = sort_dicts_by_field(fr, "order_in_video")[:max_frames]
        if not fr:
            continue
        arr = render_clip(fr, gt, pred, C, info, image_root, on_device)
        name = f"{vid}_{int(fr[0]['order_in_video'])}.gif"
        written += V.save_visualization(arr, os.path.join(str(out_dir), name), fps=fps, caption=f"{vid}", format=format)
    return written


def main(argv=None):
    p = argparse.ArgumentParser(description="ground truth, prediction and prompts of an evaluation run as 2 x 2 composites")
    p.add_argument("--gt", required=True, help="COCO annotation file of the evaluated split")
    p.add_argument("--predict", required=True, help="predict.json of the run")
    p.add_argument("--prompt", default=None, help="prompt.pkl of the run (clips and their prompts)")
    p.add_argument("--out", required=True, help="output directory")
    p.add_argument("--format", default="gif", choices=["gif", "png"])
    p.add_argument("--image-root", default=None, help="directory the images' relative paths start from")
    p.add_argument("--max-frames", type=int, default=None, help="frames per clip (default: all)")
    p.add_argument("--fps", type=int, default=4)
    p.add_argument("--host", action="store_true", help="decode and compose in numpy (no GPU)")
    a = p.parse_args(argv)
    files = visualize(a.gt, a.predict, a.out, a.prompt, a.format, a.image_root, a.max_frames, a.fps, not a.host)
    print(f"{len(files)} file(s) written to {a.out}")
    return files


if __name__ == "__main__":
    main()
