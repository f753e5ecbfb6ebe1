"""EndoVis 2018 label PNGs -> the COCO file the trainer reads (reference data/convert_endovis_to_coco.py).

A split is `<source>/<split>/images/*.png` with one class-id PNG of the same name per frame under
`<source>/<split>/annotations/`, and `<source>/labels.json` lists `{"name", "classid"}`.  Per frame and class id
> 0 one annotation: the class's mask as COCO RLE, its area and its box.  The reference does this with cv2,
pycocotools and joblib; none of them is needed here.

  * on_device=True: the label images of a chunk of frames are uploaded once, s2h_label_hist says which classes
    each frame holds (one small copy back), s2h_label_planes packs one bit plane per (frame, class),
    s2h_rle_transitions turns the planes into run boundaries, area and box, and one copy brings header and
    positions back; rle.from_transitions writes the strings.  No mask is built on the host.
  * on_device=False: numpy and rle.encode per class -- the oracle of the tests and the A/B partner.
Both write the same JSON text.

Differences from the reference: annotation PNGs are read with Pillow and must be mode "L" (cv2's grayscale
conversion of colour or palette files is not restated: such a file raises); n_jobs sizes a thread pool for the PNG
decode only.
"""
from __future__ import annotations

import argparse
import glob
import json
import os
import time
import warnings
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path
from typing import Any, Dict, List, Optional, Tuple

import numpy as np
from PIL import Image

from . import rle as _rle

_INDEX_LIMIT = 0x7FFFFFFF - 256  # F H W and P H W stay below it (s2h_label_planes)


def read_label_png(path) -> np.ndarray:
    """a class-id PNG -> uint8 [H, W]; only mode "L" is read"""
    with Image.open(path) as img:
        if img.mode != "L":
            raise ValueError(f"{path}: annotation PNG has mode {img.mode!r}; only 8-bit grayscale (mode 'L') "
                             f"label images are read")
        return np.asarray(img, dtype=np.uint8).copy()


def _box(xmin, ymin, xmax, ymax) -> List[float]:
    return [float(xmin), float(ymin), float(xmax - xmin + 1), float(ymax - ymin + 1)]


def _area_of_transitions(trans: np.ndarray, n_pixels: int) -> int:
    """the set pixels of a mask from its run boundaries: the odd runs of [0, *trans, n]"""
    b = np.concatenate([trans.astype(np.int64), [n_pixels]])
    return int((b[1::2] - b[0:-1:2][:b[1::2].size]).sum())


class EndoVisToCOCOConverter:
    """reference convert_endovis_to_coco.py:25-253"""

    def __init__(self, source_dir, output_dir, n_jobs: int = -1, on_device: bool = True,
                 frames_per_call: Optional[int] = None, planes_per_call: Optional[int] = None):
        self.source_dir = Path(source_dir)
        self.output_dir = Path(output_dir)
        self.output_dir.mkdir(exist_ok=True)
        self.n_jobs = int(n_jobs)
        self.on_device = bool(on_device)
        self.frames_per_call = frames_per_call
        self.planes_per_call = planes_per_call
        with open(self.source_dir / "labels.json") as f:
            self.class_labels = json.load(f)
        self.class_id_mapping = self.create_class_id_mapping()
        self.image_id = 0
        self.annotation_id = 0
        # seconds and bytes of the last convert_split, for A/B runs
        self.stats: Dict[str, Any] = {}

    # ------------------------------------------------------------------ the reference's small helpers
    def create_coco_categories(self) -> List[Dict]:
        return [{"id": i, "name": label["name"]} for i, label in enumerate(self.class_labels)]

    def create_class_id_mapping(self) -> Dict[int, int]:
        return {label["classid"]: i for i, label in enumerate(self.class_labels)}

    def get_image_dimensions(self, image_path) -> Tuple[int, int]:
        with Image.open(image_path) as img:
            return img.size  # (width, height)

    def extract_sequence_and_frame(self, filename: str) -> Tuple[str, int]:
        """seq_10_frame000.png -> ("seq_10_", 0)"""
        parts = filename.replace(".png", "").split("_")
        return f"{parts[0]}_{parts[1]}_", int(parts[2].replace("frame", ""))

    def workers(self) -> int:
        return min(16, os.cpu_count() or 1) if self.n_jobs < 0 else max(1, self.n_jobs)

    def _annotation(self, image_id, class_id, segmentation, area, bbox) -> Dict[str, Any]:
        return {"id": 0,  # assigned by convert_split in file order
                "image_id": image_id,
                "category_id": self.class_id_mapping.get(int(class_id), int(class_id)),
                "segmentation": segmentation,
                "area": int(area),
                "bbox": bbox,
                "iscrowd": 0}

    # ------------------------------------------------------------------ label image -> annotations
    def annotations_host(self, label: np.ndarray, image_id: int) -> List[Dict]:
        """numpy path: one annotation per class id > 0 of `label`, ascending"""
        out = []
        for c in np.unique(label):
            if c == 0:
                continue
            m = label == c
            ys, xs = np.nonzero(m)
            out.append(self._annotation(image_id, c, _rle.encode(m), m.sum(),
                                        _box(xs.min(), ys.min(), xs.max(), ys.max())))
        return out

    def annotations_device(self, labels: List[np.ndarray], image_ids: List[int], frames_per_call=None,
                           planes_per_call=None) -> List[List[Dict]]:
        """device path: the annotations of every label image, in chunks of consecutive frames of one size"""
        import torch
        from ..kernels import ops
        fpc = frames_per_call if frames_per_call is not None else self.frames_per_call
        ppc = planes_per_call if planes_per_call is not None else self.planes_per_call
        out: List[List[Dict]] = [[] for _ in labels]
        st = self.stats
        i = 0
        while i < len(labels):
            H, W = labels[i].shape
            cap = max(1, _INDEX_LIMIT // (H * W))
            nf = min(cap, 64 if fpc is None else max(1, int(fpc)))
            j = i + 1
            while j < len(labels) and j - i < nf and labels[j].shape == (H, W):
                j += 1
            t0 = time.perf_counter()
            stack = np.stack(labels[i:j])
            dev = torch.from_numpy(stack).cuda()
            hist = ops.label_hist(dev).cpu().numpy()
            st["bytes_up"] = st.get("bytes_up", 0) + stack.nbytes
            st["bytes_down"] = st.get("bytes_down", 0) + hist.nbytes
            planes = [(f, c) for f in range(j - i) for c in range(1, 256) if hist[f, c] > 0]
            np_call = min(cap, 256 if ppc is None else max(1, int(ppc)))
            for a in range(0, len(planes), np_call):
                part = planes[a:a + np_call]
                self._planes_to_annotations(ops, torch, dev, H, W, part, hist, image_ids[i:j], out, i)
            st["t_device"] = st.get("t_device", 0.0) + time.perf_counter() - t0
            i = j
        return out

    def _planes_to_annotations(self, ops, torch, dev, H, W, part, hist, image_ids, out, first):
        F, P = dev.shape[0], len(part)
        per_frame = np.bincount([f for f, _ in part], minlength=F)
        frame_off = np.concatenate([[0], np.cumsum(per_frame)]).astype(np.int32)
        plane_class = np.asarray([c for _, c in part], np.int32)
        up = torch.from_numpy(np.concatenate([frame_off, plane_class])).cuda()
        bits = ops.label_planes(dev, up[:F + 1], up[F + 1:])
        n_hdr = P * ops.RLE_HDR
        capacity = max(4096, 8 * W * P)
        buf = torch.empty(n_hdr + capacity, device=dev.device, dtype=torch.int32)
        ops.rle_transitions(bits, H, W, hdr=buf[:n_hdr], trans=buf[n_hdr:])
        a = buf.cpu().numpy()
        self.stats["bytes_up"] = self.stats.get("bytes_up", 0) + up.numel() * 4
        self.stats["bytes_down"] = self.stats.get("bytes_down", 0) + a.nbytes
        hdr, trans = a[:n_hdr].reshape(P, ops.RLE_HDR), a[n_hdr:]
        if int(hdr[0, 7]) > capacity:  # the header says how much room is needed: extract again, exactly
            _, t = ops.rle_transitions(bits, H, W, capacity=int(hdr[0, 7]))
            trans = t.cpu().numpy()
            self.stats["bytes_down"] += trans.nbytes
        for p, (f, c) in enumerate(part):
            n, off, area, xmin, ymin, xmax, ymax = (int(v) for v in hdr[p, :7])
            t = trans[off:off + n]
            decoded = _area_of_transitions(t, H * W)
            if not (area == int(hist[f, c]) == decoded):
                raise RuntimeError(f"image {image_ids[f]}, class {c}: the histogram counts {int(hist[f, c])} pixels, "
                                   f"the run header {area}, the runs {decoded}")
            out[first + f].append(self._annotation(image_ids[f], c, _rle.from_transitions(t, H, W), area,
                                                   _box(xmin, ymin, xmax, ymax)))

    def process_annotation_mask(self, mask_path, image_id: int, on_device: Optional[bool] = None) -> List[Dict]:
        """the annotations of one label PNG (reference :132-179)"""
        label = read_label_png(mask_path)
        if self.on_device if on_device is None else on_device:
            return self.annotations_device([label], [image_id])[0]
        return self.annotations_host(label, image_id)

    def image_entry(self, image_path, image_id: int) -> Dict[str, Any]:
        name = os.path.basename(image_path)
        width, height = self.get_image_dimensions(image_path)
        seq, frame = self.extract_sequence_and_frame(name)
        return {"file_name": name, "path": str(image_path), "height": height, "width": width, "id": image_id,
                "video_id": seq, "is_det_keyframe": True, "order_in_video": frame}

    def process_single_image(self, image_path, annotations_dir, base_image_id: int,
                             on_device: Optional[bool] = None):
        """(image entry, annotations), or (None, []) with a warning when the frame has no annotation file"""
        name = os.path.basename(image_path)
        annotation_path = Path(annotations_dir) / name
        if not annotation_path.exists():
            warnings.warn(f"No annotation found for {name}")
            return None, []
        return (self.image_entry(image_path, base_image_id),
                self.process_annotation_mask(annotation_path, base_image_id, on_device))

    # ------------------------------------------------------------------ splits
    def convert_split(self, split: str, on_device: Optional[bool] = None, frames_per_call=None,
                      planes_per_call=None) -> Dict[str, Any]:
        split_dir = self.source_dir / split
        images_dir, annotations_dir = split_dir / "images", split_dir / "annotations"
        if not images_dir.exists() or not annotations_dir.exists():
            raise FileNotFoundError(f"Split directory {split_dir} not found or incomplete")
        on_device = self.on_device if on_device is None else bool(on_device)
        self.stats = {"t_png": 0.0, "t_device": 0.0, "t_host": 0.0, "bytes_up": 0, "bytes_down": 0}
        coco = {"images": [], "annotations": [], "categories": self.create_coco_categories()}
        image_files = sorted(glob.glob(str(images_dir / "*.png")))
        kept = []  # (image id = index in the sorted list, image path, annotation path)
        for idx, image_path in enumerate(image_files):
            annotation_path = annotations_dir / os.path.basename(image_path)
            if not annotation_path.exists():
                warnings.warn(f"No annotation found for {os.path.basename(image_path)}")
                continue
            kept.append((self.image_id + idx, image_path, annotation_path))
        fpc = self.frames_per_call if frames_per_call is None else frames_per_call
        step = 64 if fpc is None else max(1, int(fpc))  # decoded label images held at a time
        with ThreadPoolExecutor(max_workers=self.workers()) as pool:
            for a in range(0, len(kept), step):
                part = kept[a:a + step]
                t0 = time.perf_counter()
                labels = list(pool.map(read_label_png, [k[2] for k in part]))
                entries = list(pool.map(lambda k: self.image_entry(k[1], k[0]), part))
                self.stats["t_png"] += time.perf_counter() - t0
                ids = [k[0] for k in part]
                if on_device:
                    per_image = self.annotations_device(labels, ids, fpc, planes_per_call)
                else:
                    t0 = time.perf_counter()
                    per_image = [self.annotations_host(label, i) for label, i in zip(labels, ids)]
                    self.stats["t_host"] += time.perf_counter() - t0
                for entry, annotations in zip(entries, per_image):
                    coco["images"].append(entry)
                    for ann in annotations:
                        ann["id"] = self.annotation_id
                        self.annotation_id += 1
                    coco["annotations"].extend(annotations)
        self.image_id += len(kept)
        return coco

    def convert_dataset(self):
        """both splits that exist -> endovis18_coco_annotations_{train,val}.json; ids restart per split"""
        for split in ("train", "val"):
            self.image_id = 0
            self.annotation_id = 0
            if not (self.source_dir / split).exists():
                continue
            coco = self.convert_split(split)
            output_file = self.output_dir / f"endovis18_coco_annotations_{split}.json"
            t0 = time.perf_counter()
            with open(output_file, "w") as f:
                json.dump(coco, f, indent=2)
            self.stats["t_json"] = time.perf_counter() - t0
            print(f"{split}: {len(coco['images'])} images, {len(coco['annotations'])} annotations -> {output_file}")


def main(argv=None):
    parser = argparse.ArgumentParser(description="Convert EndoVis label PNGs to the COCO file the trainer reads")
    parser.add_argument("--source_dir", type=str, required=True, help="EndoVis dataset directory (labels.json, "
                        "train/ and val/ with images/ and annotations/)")
    parser.add_argument("--output_dir", type=str, default="./", help="where the two JSON files go")
    parser.add_argument("--n_jobs", type=int, default=-1, help="threads decoding PNGs (-1: min(16, CPUs))")
    parser.add_argument("--host", action="store_true", help="numpy path instead of the device kernels")
    args = parser.parse_args(argv)
    EndoVisToCOCOConverter(args.source_dir, args.output_dir, args.n_jobs, on_device=not args.host).convert_dataset()


if __name__ == "__main__":
    main()
