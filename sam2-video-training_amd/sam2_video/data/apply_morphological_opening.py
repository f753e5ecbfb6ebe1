"""Morphological opening of every annotation of a COCO file (reference data/apply_morphological_opening.py,
which wrote the `*_opened.json` files its data configs train on).

The reference is cv2.morphologyEx(mask, MORPH_OPEN, ones((k, k))) with the default anchor and border.  Its own
output settles what that reads ("Dataset preparation"): erosion and dilation both take the offsets
-(k // 2) .. k - 1 - k // 2 along either axis, pixels outside the image ignored -- for k = 10 the windows
(-5, 4) of eval/utils.py.  `opening_window` is that rule.

Behaviour kept from the reference, quirks included: `segmentation` and `area` are replaced and `bbox` is left as
it was (the box of the mask before the opening); annotations whose opened mask is empty are removed; annotations
without a segmentation are passed through; the function that opens is called
apply_morphological_closing_to_annotations.

  * on_device=True: per chunk of annotations of one size only the run boundaries go up (s2h_rle_decode), the
    masks are eroded and dilated (s2h_morph_rect), packed (s2h_label_planes, class -1) and turned back into run
    boundaries and areas (s2h_rle_transitions); header and positions come back.  No H x W mask crosses the bus;
    `stats` counts the bytes both ways.
  * on_device=False: rle.decode, eval.utils.rect_erode / rect_dilate, rle.encode.
"""
from __future__ import annotations

import argparse
import json
import time
from typing import Any, Dict, Optional, Tuple

import numpy as np

from . import rle as _rle

MAX_REACH = 32  # ops.GP_MAX_REACH: how far a window of s2h_morph_rect reaches to either side


def opening_window(kernel_size: int) -> Tuple[int, int]:
    """(lo, hi) of the offsets a k x k window of ones reads along one axis, for the erosion and the dilation
    alike: cv2's default anchor k // 2"""
    k = int(kernel_size)
    if k < 1:
        raise ValueError(f"kernel_size {k} must be at least 1")
    if k // 2 > MAX_REACH:
        raise ValueError(f"kernel_size {k} reaches {k // 2} pixels to one side; at most {MAX_REACH} are supported")
    return -(k // 2), k - 1 - k // 2


def open_mask(mask, kernel_size: int) -> np.ndarray:
    """the opening on the host: bool [H, W]"""
    from ..eval.utils import rect_dilate, rect_erode
    win = opening_window(kernel_size)
    return rect_dilate(rect_erode(mask, win, win), win, win)


def _new_stats() -> Dict[str, Any]:
    return {"annotations": 0, "removed": 0, "bytes_up": 0, "bytes_down": 0, "t_device": 0.0, "t_host": 0.0}


def _open_chunk_device(ops, torch, counts_list, H, W, win, stats):
    """-> per annotation (area, run boundaries of the opened mask)"""
    A = len(counts_list)
    run_off, run_end = ops.rle_runs(counts_list, H, W)
    up = torch.from_numpy(np.concatenate([run_off, run_end])).cuda()
    mask = ops.rle_decode_runs(up[:A + 1], up[A + 1:], H, W)
    opened = ops.morph_rect(ops.morph_rect(mask, "erode", win, win), "dilate", win, win)
    bits = ops.mask_planes(opened)
    n_hdr = A * ops.RLE_HDR
    capacity = max(4096, int(run_end.size) + 64)  # an opening rarely adds runs; the header says when it did
    buf = torch.empty(n_hdr + capacity, device=up.device, dtype=torch.int32)
    ops.rle_transitions(bits, H, W, hdr=buf[:n_hdr], trans=buf[n_hdr:])
    a = buf.cpu().numpy()
    stats["bytes_up"] += up.numel() * 4
    stats["bytes_down"] += a.nbytes
    hdr, trans = a[:n_hdr].reshape(A, ops.RLE_HDR), a[n_hdr:]
    if int(hdr[0, 7]) > capacity:
        _, t = ops.rle_transitions(bits, H, W, capacity=int(hdr[0, 7]))
        trans = t.cpu().numpy()
        stats["bytes_down"] += trans.nbytes
    return [(int(hdr[i, 2]), trans[int(hdr[i, 1]):int(hdr[i, 1]) + int(hdr[i, 0])]) for i in range(A)]


def apply_morphological_closing_to_annotations(coco_data, kernel_size: int = 5, on_device: bool = True,
                                               anns_per_call: Optional[int] = None,
                                               stats: Optional[Dict[str, Any]] = None):
    """open every annotation's mask with a kernel_size x kernel_size window of ones, in place (the name is the
    reference's).  `stats`, when given, receives the counts, seconds and bytes_up / bytes_down of the run."""
    win = opening_window(kernel_size)
    st = _new_stats()
    anns = coco_data["annotations"]
    todo = []  # (index, h, w, counts)
    for i, ann in enumerate(anns):
        if "segmentation" not in ann or ann["segmentation"] is None:
            continue
        h, w, counts = _rle.counts_of(ann["segmentation"])
        todo.append((i, h, w, counts))
    st["annotations"] = len(todo)
    results: Dict[int, Tuple[int, Any]] = {}  # index -> (area, segmentation)
    if on_device:
        import torch
        from ..kernels import ops
        t0 = time.perf_counter()
        by_size: Dict[Tuple[int, int], list] = {}
        for item in todo:
            by_size.setdefault((item[1], item[2]), []).append(item)
        for (h, w), items in by_size.items():
            limit = max(1, (0x7FFFFFFF - 256) // (h * w))
            per = min(limit, 128 if anns_per_call is None else max(1, int(anns_per_call)))
            for a in range(0, len(items), per):
                part = items[a:a + per]
                out = _open_chunk_device(ops, torch, [it[3] for it in part], h, w, win, st)
                for it, (area, trans) in zip(part, out):
                    results[it[0]] = (area, _rle.from_transitions(trans, h, w) if area else None)
        st["t_device"] = time.perf_counter() - t0
    else:
        t0 = time.perf_counter()
        for i, h, w, counts in todo:
            opened = open_mask(_rle.decode({"size": [h, w], "counts": counts}), kernel_size)
            area = int(opened.sum())
            results[i] = (area, _rle.encode(opened) if area else None)
        st["t_host"] = time.perf_counter() - t0
    remove = []
    for i, (area, seg) in results.items():
        if area == 0:
            remove.append(i)
            continue
        anns[i]["segmentation"] = seg
        anns[i]["area"] = area
    for i in sorted(remove, reverse=True):
        del anns[i]
    st["removed"] = len(remove)
    if stats is not None:
        stats.update(st)
    return coco_data


def process_coco_file(input_path, output_path, kernel_size: int = 10, on_device: bool = True,
                      anns_per_call: Optional[int] = None) -> Dict[str, Any]:
    """input JSON -> output JSON with every annotation opened; -> the run's stats (see above)"""
    t0 = time.perf_counter()
    with open(input_path) as f:
        coco_data = json.load(f)
    t_load = time.perf_counter() - t0
    original = len(coco_data["annotations"])
    stats: Dict[str, Any] = {}
    apply_morphological_closing_to_annotations(coco_data, kernel_size, on_device=on_device,
                                               anns_per_call=anns_per_call, stats=stats)
    t0 = time.perf_counter()
    with open(output_path, "w") as f:
        json.dump(coco_data, f, indent=2)
    stats["t_json"] = t_load + time.perf_counter() - t0
    print(f"{input_path}: {original} annotations, {stats['removed']} emptied by the opening and removed "
          f"-> {output_path}")
    return stats


def main(argv=None):
    parser = argparse.ArgumentParser(description="Open every annotation mask of a COCO file (k x k window of ones)")
    parser.add_argument("input", help="COCO JSON to read")
    parser.add_argument("output", help="COCO JSON to write")
    parser.add_argument("--kernel-size", type=int, default=10)
    parser.add_argument("--host", action="store_true", help="numpy path instead of the device kernels")
    args = parser.parse_args(argv)
    process_coco_file(args.input, args.output, args.kernel_size, on_device=not args.host)


if __name__ == "__main__":
    main()
