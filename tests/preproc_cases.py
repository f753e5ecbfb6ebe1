"""Shared by test_preproc_host.py and test_preproc_gpu.py: a numpy model of Pillow's two-pass resample driven by
ops.resample_taps, the case files of csrc/preproc_host_check.cpp, annotation sets for the category masks and a
tiny COCO clip set written into a directory."""
import json
import os

import numpy as np

from sam2_video.data import rle

RESIZE_SHAPES = [((37, 53), (16, 22)), ((19, 23), (64, 77)), ((64, 48), (32, 32)), ((31, 17), (32, 32)),
                 ((1024, 1280), (512, 640))]


def test_image(H, W, kind, seed=0):
    """uint8 [H, W, 3]: uniform noise ("random") or a smooth pattern with a few hard edges ("smooth")"""
    rng = np.random.default_rng(seed)
    if kind == "random":
        return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    yy, xx = np.mgrid[:H, :W].astype(np.float64)
    img = np.stack([127.5 + 127.5 * np.sin(xx / 7.0 + yy / 11.0), 255.0 * xx / max(W - 1, 1),
                    255.0 * ((yy // 5 + xx // 9) % 2)], axis=-1)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def model_axis(img, taps, axis):
    """one pass of the resample along `axis` with the tables of ops.resample_taps, in int64"""
    xmin, cnt, coef = taps
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.zeros((len(xmin),) + src.shape[1:], np.int64)
    for o in range(len(xmin)):
        acc = np.tensordot(coef[o, :cnt[o]].astype(np.int64), src[xmin[o]:xmin[o] + cnt[o]], axes=(0, 0))
        out[o] = np.clip((acc + (1 << 21)) >> 22, 0, 255)
    return np.moveaxis(out, 0, axis).astype(np.uint8)


def model_resize(arr, nh, nw, filt):
    """Image.resize((nw, nh), filt) on uint8 [H, W, 3]: horizontal pass, then vertical"""
    from sam2_video.kernels import ops
    h, w = arr.shape[:2]
    mid = model_axis(arr, ops.resample_taps(w, nw, filt), 1)
    return model_axis(mid, ops.resample_taps(h, nh, filt), 0)


def write_cases(path, cases):
    """cases: [(header ints, [arrays])] in the layout preproc_host_check reads"""
    with open(path, "wb") as f:
        for hdr, arrays in cases:
            f.write(np.asarray(list(hdr) + [0] * (12 - len(hdr)), np.int32).tobytes())
            for a in arrays:
                f.write(np.ascontiguousarray(a).tobytes())


def resample_case(frames, out_hw, top_left, crop_hw, filt, lut):
    """the arguments s2h_resample_u8_norm gets from ops.resample_u8_norm, as a host-check case"""
    from sam2_video.kernels import ops
    F, H, W, _ = frames.shape
    (nh, nw), (top, left), (ch, cw) = out_hw, top_left, crop_hw
    xm, xc, xk = ops.resample_taps(W, nw, filt)
    ym, yc, yk = ops.resample_taps(H, nh, filt)
    ym, yc, yk = ym[top:top + ch], yc[top:top + ch], yk[top:top + ch]
    row0 = int(ym.min())
    nrows = int((ym + yc).max()) - row0
    hdr = (0, F, H, W, cw, xk.shape[1], ch, yk.shape[1], row0, nrows)
    return hdr, [frames, xm[left:left + cw], xc[left:left + cw], xk[left:left + cw], ym, yc, yk,
                 np.asarray(lut, np.float32)]


# ------------------------------------------------------------------------------------------- category masks
def blob(H, W, cy, cx, ry, rx):
    yy, xx = np.mgrid[:H, :W]
    return (((yy - cy) / max(ry, 0.5)) ** 2 + ((xx - cx) / max(rx, 0.5)) ** 2 <= 1.0).astype(np.uint8)


def catmask_frames(H, W, N):
    """two frames of annotations [(category index, mask uint8 [H, W])], different counts per frame: two
    overlapping annotations of one category, a category without annotation, a category index out of range
    (-1), a mask that starts set (first count 0), an empty annotation"""
    rng = np.random.default_rng(H * 1000 + W)
    full_col = np.zeros((H, W), np.uint8)
    full_col[:, 0] = 1                       # starts set: the first count is 0
    full_col[: max(1, H // 2), W - 1] = 1
    noise = (rng.random((H, W)) < 0.3).astype(np.uint8)
    f0 = [(0, blob(H, W, H * 0.4, W * 0.4, H * 0.25, W * 0.2)), (0, blob(H, W, H * 0.5, W * 0.55, H * 0.2, W * 0.25)),
          (2 % N, full_col), (-1, np.ones((H, W), np.uint8)), (N - 1, np.zeros((H, W), np.uint8)),
          (3 % N, noise)]
    f1 = [(N - 1, blob(H, W, H * 0.7, W * 0.3, H * 0.2, W * 0.2)), (0, np.ones((H, W), np.uint8))]
    if N >= 64:  # every plane of the 64-bit set, the top one included
        f1 += [(n, (rng.random((H, W)) < 0.5).astype(np.uint8)) for n in range(N)]
    return [f0, f1]


def runs_of(frames, H, W):
    """-> (run_off, run_end, ann_cat, frame_off) int32 numpy, the annotations of all frames back to back"""
    from sam2_video.kernels import ops
    counts, cats, foff = [], [], [0]
    for anns in frames:
        for c, m in anns:
            counts.append(rle.counts_from_string(rle.encode(m)["counts"]))
            cats.append(c)
        foff.append(len(cats))
    run_off, run_end = ops.rle_runs(counts, H, W)
    return run_off, run_end, np.asarray(cats, np.int32), np.asarray(foff, np.int32)


def dense_catmasks(frames, N, S):
    """what COCOImageDataset._load_gt_masks_for_image computes: resize_mask(rle.decode(.)) OR-ed per category"""
    import torch
    from sam2_video.data import dataset as D
    out = torch.zeros(len(frames), N, S, S, dtype=torch.bool)
    for f, anns in enumerate(frames):
        for c, m in anns:
            if 0 <= c < N:
                out[f, c] |= D.resize_mask(rle.decode(rle.encode(m)), S)
    return out


# ------------------------------------------------------------------------------------------- a tiny COCO set
def write_coco(root, T, H, W, N, S, empty=(), clip=None, seed=0):
    """T frames of one video (PNG files, lossless) with 1-3 annotations each; the images listed in `empty` have
    only annotations that miss every sampled position.  -> (json path, data config dict)"""
    from PIL import Image
    rng = np.random.default_rng(seed)
    os.makedirs(root, exist_ok=True)
    images, anns = [], []
    for t in range(T):
        path = os.path.join(root, f"{t}.png")
        Image.fromarray(test_image(H, W, "random" if t % 2 else "smooth", seed + t)).save(path)
        images.append({"id": 100 + t, "path": path, "is_det_keyframe": True, "video_id": 7, "order_in_video": t,
                       "height": H, "width": W})
        if t in empty:
            continue
        for k in range(1 + t % 3):
            m = blob(H, W, rng.uniform(0.3, 0.7) * H, rng.uniform(0.3, 0.7) * W, rng.uniform(0.1, 0.3) * H,
                     rng.uniform(0.1, 0.3) * W)
            anns.append({"id": len(anns), "image_id": 100 + t, "category_id": 10 * (1 + (t + k) % N),
                         "segmentation": rle.encode(m)})
    anns.append({"id": len(anns), "image_id": 100, "category_id": 999, "segmentation": rle.encode(np.ones((H, W)))})
    coco = {"images": images, "annotations": anns, "categories": [{"id": 10 * (n + 1)} for n in range(N)]}
    jp = os.path.join(root, "coco.json")
    with open(jp, "w") as f:
        json.dump(coco, f)
    cfg = {"train_path": jp, "image_size": S, "num_categories": N, "video_clip_length": clip or T, "stride": 1}
    return jp, cfg
