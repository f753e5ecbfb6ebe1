"""The shared cases of the dataset-preparation kernels (s2h_label_hist / s2h_label_planes): label images, the
plane lists a converter would ask for, and the numpy reference.  Used by test_dataprep_host.py (the host replay
of the kernels' decomposition) and test_dataprep_gpu.py (the kernels)."""
import numpy as np

from sam2_video.kernels import ops

# (H, W): one pixel; 65 positions = one position into a second word; its transpose; whole words per column;
# every word straddles a column; more than two bands of 64 columns with the last one partial; several 64-word
# wave chunks per band ... and the two sizes at which s2h_label_planes takes another path: a staged tile above
# 64 KB (H > 1024) and the direct form (H > DP_STAGED_MAX_H = 2048)
SIZES = [(1, 1), (5, 13), (13, 5), (64, 3), (65, 3), (63, 130), (96, 40), (1100, 3), (2050, 2)]
FRAMES = [1, 3]
CONTENTS = ["background", "full", "value255", "checker", "blocks", "neighbours", "bytes"]
HIST_BIG = (300, 300)  # 90 000 pixels of one value: a 16-bit counter overflows


def _frame(kind, f, H, W, rng):
    y, x = np.mgrid[0:H, 0:W]
    if kind == "background":
        return np.zeros((H, W), np.uint8)
    if kind == "full":
        return np.full((H, W), 5, np.uint8)
    if kind == "value255":
        return np.where((y + 2 * x + f) % 3 == 0, 255, 0).astype(np.uint8)
    if kind == "checker":  # the most transitions possible, no background
        return (1 + (y + x + f) % 2).astype(np.uint8)
    if kind == "blocks":  # four classes in blocks, background between them where there is room
        cls = np.asarray([1, 2, 3, 200], np.uint8)[(2 * (y >= (H + 1) // 2) + (x >= (W + 1) // 2))]
        gap = (y == H // 3) & (H > 3) | (x == W // 3) & (W > 3)
        return np.where(gap, 0, cls).astype(np.uint8)
    if kind == "neighbours":  # frame 0: {1, 2}, frame 1: nothing, frame 2: {3, 7, 9}
        if f % 3 == 1:
            return np.zeros((H, W), np.uint8)
        vals = np.asarray([0, 1, 2], np.uint8) if f % 3 == 0 else np.asarray([0, 3, 7, 9], np.uint8)
        return vals[rng.integers(0, vals.size, size=(H, W))]
    if kind == "bytes":  # byte masks for the -1 form
        return np.asarray([0, 1, 7, 255], np.uint8)[rng.integers(0, 4, size=(H, W))]
    raise ValueError(kind)


def make_case(name, labels, mask_form=False):
    """labels [F, H, W] uint8 -> the case: one plane per (frame, class > 0) in ascending class order, or one
    plane of class -1 per frame (`mask_form`)"""
    labels = np.ascontiguousarray(labels, np.uint8)
    frame_off, plane_class = [0], []
    for img in labels:
        plane_class += [-1] if mask_form else [int(c) for c in np.unique(img) if c > 0]
        frame_off.append(len(plane_class))
    return {"name": name, "labels": labels, "frame_off": np.asarray(frame_off, np.int32),
            "plane_class": np.asarray(plane_class, np.int32)}


def make_cases():
    rng = np.random.default_rng(20181)
    cases = []
    for H, W in SIZES:
        for F in FRAMES:
            for kind in CONTENTS:
                if kind == "neighbours" and F == 1:
                    continue
                labels = np.stack([_frame(kind, f, H, W, rng) for f in range(F)])
                cases.append(make_case(f"{H}x{W}-F{F}-{kind}", labels, mask_form=kind == "bytes"))
    cases.append(make_case("hist_big", np.full((1,) + HIST_BIG, 3, np.uint8)))
    return cases


def reference(case):
    """-> (hist int32 [F, 256], bits int64 [P, ceil(H W / 64)]) from np.bincount and ops.pack_mask_bits"""
    labels = case["labels"]
    F, H, W = labels.shape
    hist = np.stack([np.bincount(img.reshape(-1), minlength=256) for img in labels]).astype(np.int32)
    planes = []
    for f in range(F):
        for p in range(case["frame_off"][f], case["frame_off"][f + 1]):
            c = int(case["plane_class"][p])
            planes.append(labels[f] != 0 if c == -1 else labels[f] == c)
    if planes:
        bits = ops.pack_mask_bits(np.stack(planes))
    else:
        bits = np.zeros((0, ops.rle_words(H, W)), np.int64)
    return hist, bits


# ------------------------------------------------------------------ the synthetic EndoVis tree of the tool tests
TREE_H, TREE_W = 96, 80
TREE_LABELS = [{"name": "shaft", "classid": 3}, {"name": "wrist", "classid": 7}, {"name": "thread", "classid": 200}]


def _tree_label(kind, rng):
    """label images whose classes are solid blocks (they survive a 10 x 10 opening), thin bars and specks (they
    do not), with ragged edges"""
    H, W = TREE_H, TREE_W
    m = np.zeros((H, W), np.uint8)
    if kind == "background":
        return m
    m[8:40, 6:30] = 3
    m[50:90, 40:76] = 7
    m[0:14, 60:80] = 200           # touches two borders
    m[44:47, 2:38] = 200           # a bar 3 pixels high: opened away at k = 10, a second piece of class 200
    noise = rng.random((H, W)) < 0.04
    m[noise & (m != 0)] = 0        # holes
    if kind == "unlisted":
        m[70:76, 4:9] = 9          # a class labels.json does not list; 6 x 5: emptied by the opening
    if kind == "thin":             # only pieces the opening removes: the frame stops being a keyframe
        m[:] = 0
        m[10:13, 5:60] = 3
        m[30:70, 20:24] = 7
    return m


def build_tree(root, with_rgb=False):
    """write the tree under `root` (a pathlib.Path) -> {split: [(file name, label uint8 [H, W] or None)]}, the
    files sorted; None = the frame has no annotation file"""
    from PIL import Image
    import json
    rng = np.random.default_rng(96080)
    plan = {"train": [("seq_1_frame000.png", "blocks"), ("seq_1_frame001.png", "unlisted"),
                      ("seq_1_frame002.png", None), ("seq_1_frame003.png", "background"),
                      ("seq_1_frame004.png", "thin"), ("seq_2_frame000.png", "blocks")],
            "val": [("seq_3_frame010.png", "blocks"), ("seq_3_frame011.png", "unlisted")]}
    root.mkdir(parents=True, exist_ok=True)
    (root / "labels.json").write_text(json.dumps(TREE_LABELS))
    tree = {}
    for split, frames in plan.items():
        (root / split / "images").mkdir(parents=True)
        (root / split / "annotations").mkdir(parents=True)
        tree[split] = []
        for name, kind in frames:
            rgb = rng.integers(0, 256, size=(TREE_H, TREE_W, 3), dtype=np.uint8)
            Image.fromarray(rgb, "RGB").save(root / split / "images" / name)
            label = None if kind is None else _tree_label(kind, rng)
            if label is not None:
                Image.fromarray(label, "L").save(root / split / "annotations" / name)
            tree[split].append((name, label))
    if with_rgb:
        name = "seq_9_frame000.png"
        rgb = np.zeros((TREE_H, TREE_W, 3), np.uint8)
        Image.fromarray(rgb, "RGB").save(root / "train" / "images" / name)
        Image.fromarray(rgb, "RGB").save(root / "train" / "annotations" / name)
    return tree


def expected_coco(root, tree, split):
    """what the converter must write for `split`, from numpy and rle.encode"""
    from sam2_video.data import rle
    cat_of = {label["classid"]: i for i, label in enumerate(TREE_LABELS)}
    coco = {"images": [], "annotations": [], "categories": [{"id": i, "name": label["name"]}
                                                             for i, label in enumerate(TREE_LABELS)]}
    for idx, (name, label) in enumerate(tree[split]):
        if label is None:
            continue  # its index stays unused
        seq, frame = name[:-4].rsplit("_", 1)
        coco["images"].append({"file_name": name, "path": str(root / split / "images" / name), "height": TREE_H,
                               "width": TREE_W, "id": idx, "video_id": seq + "_", "is_det_keyframe": True,
                               "order_in_video": int(frame[len("frame"):])})
        for c in sorted(int(v) for v in np.unique(label) if v > 0):
            m = label == c
            ys, xs = np.nonzero(m)
            coco["annotations"].append({
                "id": len(coco["annotations"]), "image_id": idx, "category_id": cat_of.get(c, c),
                "segmentation": rle.encode(m), "area": int(m.sum()),
                "bbox": [float(xs.min()), float(ys.min()), float(xs.max() - xs.min() + 1),
                         float(ys.max() - ys.min() + 1)], "iscrowd": 0})
    return coco


def paint_fixture(root, fixture):
    """the golden's three images as a tree: the label image is painted from the decoded masks with class id =
    category + 1 -> (tree root, {file name: the golden's annotations of that image, by category id})"""
    import json
    from PIL import Image
    from sam2_video.data import rle
    n_cat = len(fixture["categories"])
    root.mkdir(parents=True, exist_ok=True)
    (root / "labels.json").write_text(json.dumps([{"name": c["name"], "classid": c["id"] + 1}
                                                  for c in fixture["categories"]]))
    (root / "val" / "images").mkdir(parents=True)
    (root / "val" / "annotations").mkdir(parents=True)
    want = {}
    for img in fixture["images"]:
        label = np.zeros((img["height"], img["width"]), np.uint8)
        want[img["file_name"]] = {}
        for a in fixture["annotations"]:
            if int(a["image_id"]) != int(img["id"]):
                continue
            cat = int(a["category_id"])
            assert 0 <= cat < n_cat
            label[rle.decode(a["segmentation"]).astype(bool)] = cat + 1
            want[img["file_name"]][cat] = a
        Image.fromarray(label, "L").save(root / "val" / "annotations" / img["file_name"])
        Image.new("RGB", (img["width"], img["height"])).save(root / "val" / "images" / img["file_name"])
    return want


def check_fixture_output(coco, want):
    """the converter's annotations equal the golden's (written by pycocotools) per image, keyed by category"""
    import ast
    from sam2_video.data import rle
    name_of = {img["id"]: img["file_name"] for img in coco["images"]}
    assert sorted(name_of.values()) == sorted(want)
    seen = {name: set() for name in want}
    for ann in coco["annotations"]:
        name = name_of[ann["image_id"]]
        ref = want[name][ann["category_id"]]
        seen[name].add(ann["category_id"])
        ref_seg = rle._as_rle(ref["segmentation"])
        assert ann["segmentation"] == {"size": list(ref_seg["size"]), "counts": ref_seg["counts"]}, (name, ann["category_id"])
        assert ann["area"] == int(ref["area"])
        ref_box = ref["bbox"] if not isinstance(ref["bbox"], str) else ast.literal_eval(ref["bbox"])
        assert ann["bbox"] == [float(v) for v in ref_box]
        assert ann["iscrowd"] == int(ref["iscrowd"]) == 0
    assert all(seen[name] == set(want[name]) for name in want)
