"""A/B of the dataset-preparation tools: the host numpy path of this build against the device path of this build,
in one process, on a generated 1024 x 1280 EndoVis-like tree (default 200 frames with 3-4 classes each, so about
700 annotations for the opening).  Prints wall times, bytes moved and the share spent in PNG decode / JSON
encode; there is no other implementation on this machine to compare with (the reference's scripts need cv2 and
pycocotools).

    python tools/dataprep_ab.py [--frames 200] [--out DIR]
"""
import argparse
import json
import os
import sys
import tempfile
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sam2-video-training_amd"))

H, W = 1024, 1280


def make_tree(root, frames, rng):
    from PIL import Image
    os.makedirs(os.path.join(root, "train", "images"))
    os.makedirs(os.path.join(root, "train", "annotations"))
    classes = [1, 2, 3, 4, 5, 6, 7]
    with open(os.path.join(root, "labels.json"), "w") as f:
        json.dump([{"name": f"c{c}", "classid": c} for c in classes], f)
    yy, xx = np.mgrid[0:H, 0:W]
    blank = Image.new("RGB", (W, H))
    for i in range(frames):
        label = np.zeros((H, W), np.uint8)
        for c in rng.choice(classes, size=3 + i % 2, replace=False):  # tool-like blobs: slanted bars with ragged edges
            cy, cx, a = rng.integers(100, H - 100), rng.integers(100, W - 100), rng.uniform(-1.2, 1.2)
            d = (yy - cy) * np.cos(a) - (xx - cx) * np.sin(a)
            along = (yy - cy) * np.sin(a) + (xx - cx) * np.cos(a)
            label[(np.abs(d) < rng.integers(20, 90)) & (np.abs(along) < rng.integers(150, 500))] = c
        label[rng.random((H, W)) < 0.002] = 0
        name = f"seq_{1 + i // 50}_frame{i % 50:03d}.png"
        Image.fromarray(label, "L").save(os.path.join(root, "train", "annotations", name))
        blank.save(os.path.join(root, "train", "images", name))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from sam2_video.data import apply_morphological_opening as OPEN
    from sam2_video.data import convert_endovis_to_coco as CONV
    from sam2_video.kernels import ops
    warnings.simplefilter("ignore")
    work = args.out or tempfile.mkdtemp(prefix="dataprep_ab_")
    src = os.path.join(work, "src")
    make_tree(src, args.frames, np.random.default_rng(7))
    ops.label_hist(torch.zeros(1, 8, 8, dtype=torch.uint8, device="cuda"))  # load the library, start the device
    torch.cuda.synchronize()
    print(f"host numpy path of this build vs device path of this build; {args.frames} frames of {H} x {W}, "
          f"{torch.cuda.get_device_name(0)}")
    texts = {}
    for on_device in (False, True):
        out = os.path.join(work, "dev" if on_device else "host")
        conv = CONV.EndoVisToCOCOConverter(src, out, on_device=on_device)
        t0 = time.perf_counter()
        conv.convert_dataset()
        if on_device:
            torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        s = conv.stats
        path = os.path.join(out, "endovis18_coco_annotations_train.json")
        texts[on_device] = open(path).read()
        n_ann = len(json.loads(texts[on_device])["annotations"])
        work_t = s["t_device"] if on_device else s["t_host"]
        print(f"convert  on_device={on_device!s:5}: wall {wall:7.2f} s = PNG decode {s['t_png']:.2f} s "
              f"({100 * s['t_png'] / wall:.0f}%) + masks to RLE {work_t:.2f} s + JSON write {s['t_json']:.2f} s "
              f"({100 * s['t_json'] / wall:.0f}%); {n_ann} annotations; up {s['bytes_up']} B, down {s['bytes_down']} B")
    print("convert: same text", texts[True] == texts[False])
    src_json = os.path.join(work, "host", "endovis18_coco_annotations_train.json")
    for on_device in (False, True):
        dst = os.path.join(work, f"opened_{'dev' if on_device else 'host'}.json")
        t0 = time.perf_counter()
        s = OPEN.process_coco_file(src_json, dst, kernel_size=10, on_device=on_device)
        wall = time.perf_counter() - t0
        work_t = s["t_device"] if on_device else s["t_host"]
        texts[on_device] = open(dst).read()
        print(f"opening  on_device={on_device!s:5}: wall {wall:7.2f} s = opening {work_t:.2f} s + JSON read and write "
              f"{s['t_json']:.2f} s ({100 * s['t_json'] / wall:.0f}%); {s['annotations']} annotations, {s['removed']} "
              f"removed; up {s['bytes_up']} B, down {s['bytes_down']} B "
              f"(one byte mask: {H * W} B)")
    print("opening: same text", texts[True] == texts[False])


if __name__ == "__main__":
    main()
