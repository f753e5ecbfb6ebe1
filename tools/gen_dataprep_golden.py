"""TEST INFRASTRUCTURE ONLY -- one-off extraction of tests/golden/dataprep_endovis18_images.json from the
reference's own annotation file (data/endovis18.json, which pycocotools wrote): the image entries, the
annotations verbatim and the categories of three images that have four annotations each.  The converter tests
paint a label image from the decoded masks (class id = category + 1), convert it, and expect these
annotations back.  Reads data only; never run by a test.

    python tools/gen_dataprep_golden.py <reference checkout>/data/endovis18.json
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sam2-video-training_amd"))
OUT = os.path.join(ROOT, "tests", "golden", "dataprep_endovis18_images.json")
LIMIT = 64 * 1024


def main(src, n_images=3, n_anns=4):
    import numpy as np
    from sam2_video.data import rle
    coco = json.load(open(src))
    by_image = {}
    for ann in coco["annotations"]:
        by_image.setdefault(ann["image_id"], []).append(ann)
    images, annotations = [], []
    for img in coco["images"]:
        anns = by_image.get(str(img["id"]), by_image.get(img["id"], []))
        if len(anns) != n_anns or len({a["category_id"] for a in anns}) != n_anns:
            continue
        cover = np.zeros((img["height"], img["width"]), np.int32)
        for a in anns:
            cover += rle.decode(a["segmentation"])
        if cover.max() > 1:  # overlapping masks cannot be painted into one label image
            continue
        images.append(img)
        annotations += anns
        if len(images) == n_images:
            break
    assert len(images) == n_images
    for img in images:  # the images' masks are disjoint
        total = sum(int(rle.decode(a["segmentation"]).sum()) for a in annotations if a["image_id"] == str(img["id"]))
        union = np.zeros((img["height"], img["width"]), bool)
        for a in annotations:
            if a["image_id"] == str(img["id"]):
                union |= rle.decode(a["segmentation"]).astype(bool)
        assert int(union.sum()) == total, f"image {img['id']}: its masks overlap"
    out = {"images": images, "annotations": annotations, "categories": coco["categories"]}
    with open(OUT, "w") as f:
        json.dump(out, f)
    size = os.path.getsize(OUT)
    assert size < LIMIT, size
    print(OUT, size)


if __name__ == "__main__":
    main(sys.argv[1])
