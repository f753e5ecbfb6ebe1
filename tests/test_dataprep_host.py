"""Dataset preparation without a GPU: csrc/dataprep.h compiled for the host and run in the kernels' decomposition
(csrc/dataprep_host_check.cpp: a stand-alone program, built plain and under the address and undefined-behaviour
sanitizers) against numpy on every case of dataprep_cases.py, and the host paths of the three tools
(sam2_video/data/convert_endovis_to_coco.py, apply_morphological_opening.py, update_is_det_keyframe.py) on a
synthetic tree, on the reference's own opened masks and on three of its converted images."""
import copy
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import dataprep_cases as DC
from sam2_video.data import apply_morphological_opening as OPEN
from sam2_video.data import convert_endovis_to_coco as CONV
from sam2_video.data import rle
from sam2_video.data import update_is_det_keyframe as KEY
from sam2_video.eval.utils import rect_dilate, rect_erode
from sam2_video.kernels import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sam2-video-training_amd")
CSRC = os.path.join(PKG, "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden")


# ------------------------------------------------------------------------------ the kernels' host model
@pytest.fixture(scope="module")
def cases():
    cs = DC.make_cases()
    return cs, [DC.reference(c) for c in cs]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def host_check(request, tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build csrc/dataprep_host_check.cpp")
    exe = tmp_path_factory.mktemp("dataprep_host") / f"dataprep_host_check_{request.param}"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", *flags, "-I", CSRC,
                    os.path.join(CSRC, "dataprep_host_check.cpp"), "-o", str(exe)], check=True)
    return str(exe)


def _case_bytes(F, H, W, labels, frame_off, plane_class):
    return (np.asarray([F, H, W, len(plane_class)], np.int32).tobytes() + np.asarray(labels, np.uint8).tobytes()
            + np.asarray(frame_off, np.int32).tobytes() + np.asarray(plane_class, np.int32).tobytes())


def run_host(exe, cases, tmp_path):
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        for c in cases:
            f.write(_case_bytes(*c["labels"].shape, c["labels"], c["frame_off"], c["plane_class"]))
    subprocess.run([exe, str(src), str(dst)], check=True, timeout=300)
    raw, out, off = dst.read_bytes(), [], 0
    for c in cases:
        F, H, W = c["labels"].shape
        P, nw = c["plane_class"].size, ops.rle_words(H, W)
        hist = np.frombuffer(raw, np.int32, F * 256, off).reshape(F, 256)
        off += F * 256 * 4
        bits = np.frombuffer(raw, np.int64, P * nw, off).reshape(P, nw)
        off += P * nw * 8
        out.append((hist, bits))
    assert off == len(raw)
    return out


def test_the_cases_cover_what_they_claim(cases):
    cs, refs = cases
    by_name = {c["name"]: (c, r) for c, r in zip(cs, refs)}
    assert {c["labels"].shape[1:] for c in cs} == set(DC.SIZES) | {DC.HIST_BIG}
    assert {c["labels"].shape[0] for c in cs} == {1, 3}
    assert 5 * 13 == 65 and 65 % 64 != 0  # one position into a second word; words straddle columns
    for H, W in DC.SIZES:
        c, (hist, bits) = by_name[f"{H}x{W}-F3-background"]
        assert c["plane_class"].size == 0 and (hist[:, 0] == H * W).all() and bits.shape[0] == 0
        c, (hist, bits) = by_name[f"{H}x{W}-F1-full"]
        assert list(c["plane_class"]) == [5] and hist[0, 5] == H * W
        c, _ = by_name[f"{H}x{W}-F3-value255"]
        assert 255 in c["plane_class"]
        c, _ = by_name[f"{H}x{W}-F1-checker"]
        assert (c["labels"] > 0).all() and (H * W == 1 or set(c["plane_class"]) == {1, 2})
        c, _ = by_name[f"{H}x{W}-F3-neighbours"]
        per_frame = np.diff(c["frame_off"])
        assert per_frame[1] == 0  # a frame without planes between two that have some
        c, _ = by_name[f"{H}x{W}-F3-bytes"]
        assert (c["plane_class"] == -1).all() and c["plane_class"].size == 3
    c, _ = by_name["96x40-F1-blocks"]
    assert list(c["plane_class"]) == [1, 2, 3, 200]
    assert by_name["96x40-F3-neighbours"][0]["plane_class"].tolist() == [1, 2, 3, 7, 9]
    assert by_name["hist_big"][1][0][0, 3] == 90000 > 0xFFFF
    assert max(H for H, _ in DC.SIZES) > 2048 and any(1024 < H <= 2048 for H, _ in DC.SIZES)  # the three paths


def test_host_model_equals_numpy(host_check, cases, tmp_path):
    cs, refs = cases
    got = run_host(host_check, cs, tmp_path)
    for c, (hist, bits), (want_hist, want_bits) in zip(cs, got, refs):
        assert (hist == want_hist).all(), c["name"]
        assert bits.shape == want_bits.shape and (bits == want_bits).all(), c["name"]


def test_host_check_refuses_sizes_beyond_the_limits(host_check, tmp_path):
    dst = tmp_path / "out.bin"
    for n, (F, H, W, P) in enumerate([(1, 0, 4, 0), (1, 4, 0, 0), (1, 4097, 4096, 0), (-1, 2, 2, 0),
                                      (200, 4096, 4096, 0), (1, 4096, 4096, 200)]):
        src = tmp_path / f"in{n}.bin"
        src.write_bytes(np.asarray([F, H, W, P], np.int32).tobytes())
        assert subprocess.run([host_check, str(src), str(dst)], timeout=60).returncode == 3, (F, H, W, P)
    src = tmp_path / "csr.bin"  # frame_off does not end at P
    src.write_bytes(_case_bytes(1, 2, 2, np.ones(4, np.uint8), [0, 2], [1]))
    assert subprocess.run([host_check, str(src), str(dst)], timeout=60).returncode == 3


# ------------------------------------------------------------------------------ the tools, host paths
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = tmp_path_factory.mktemp("endovis") / "src"
    return root, DC.build_tree(root)


@pytest.fixture(scope="module")
def converted(tree, tmp_path_factory):
    root, _ = tree
    out = tmp_path_factory.mktemp("coco_host")
    with pytest.warns(UserWarning, match="No annotation found for seq_1_frame002.png"):
        CONV.EndoVisToCOCOConverter(root, out, n_jobs=2, on_device=False).convert_dataset()
    return out


def test_converter_writes_the_expected_files(tree, converted):
    root, t = tree
    for split in ("train", "val"):
        text = (converted / f"endovis18_coco_annotations_{split}.json").read_text()
        want = DC.expected_coco(root, t, split)
        assert text == json.dumps(want, indent=2)  # values, key order and indentation
        got = json.loads(text)
        assert list(got) == ["images", "annotations", "categories"]
        assert list(got["images"][0]) == ["file_name", "path", "height", "width", "id", "video_id", "is_det_keyframe",
                                          "order_in_video"]
        assert [a["id"] for a in got["annotations"]] == list(range(len(got["annotations"])))  # restart per split
        assert all(isinstance(a["area"], int) and all(isinstance(v, float) for v in a["bbox"]) and a["iscrowd"] == 0
                   for a in got["annotations"])
    train = json.loads((converted / "endovis18_coco_annotations_train.json").read_text())
    assert [i["id"] for i in train["images"]] == [0, 1, 3, 4, 5]  # index 2 has no annotation file: unused
    assert train["images"][0]["video_id"] == "seq_1_" and train["images"][-1]["video_id"] == "seq_2_"
    assert [i["order_in_video"] for i in train["images"]] == [0, 1, 3, 4, 0]
    assert [a["category_id"] for a in train["annotations"] if a["image_id"] == 1] == [0, 1, 9, 2]  # 3, 7, 9, 200
    assert not [a for a in train["annotations"] if a["image_id"] == 3]  # all background
    assert train["categories"] == [{"id": 0, "name": "shaft"}, {"id": 1, "name": "wrist"}, {"id": 2, "name": "thread"}]


def test_converter_single_image_entry_points(tree, tmp_path):
    root, t = tree
    conv = CONV.EndoVisToCOCOConverter(root, tmp_path / "o", on_device=False)
    ann_dir = root / "train" / "annotations"
    entry, anns = conv.process_single_image(str(root / "train" / "images" / "seq_1_frame001.png"), ann_dir, 41)
    assert entry["id"] == 41 and [a["image_id"] for a in anns] == [41] * 4
    assert anns == conv.process_annotation_mask(ann_dir / "seq_1_frame001.png", 41)
    with pytest.warns(UserWarning, match="No annotation found"):
        assert conv.process_single_image(str(root / "train" / "images" / "seq_1_frame002.png"), ann_dir, 2) == (None, [])
    assert conv.workers() == min(16, os.cpu_count() or 1)
    assert CONV.EndoVisToCOCOConverter(root, tmp_path / "o", n_jobs=3, on_device=False).workers() == 3
    with pytest.raises(FileNotFoundError):
        conv.convert_split("test")


def test_converter_rejects_a_colour_annotation(tmp_path):
    root = tmp_path / "src"
    DC.build_tree(root, with_rgb=True)
    conv = CONV.EndoVisToCOCOConverter(root, tmp_path / "out", on_device=False)
    with pytest.raises(ValueError, match=r"seq_9_frame000\.png.*'RGB'"), pytest.warns(UserWarning):
        conv.convert_split("train")


def _anns(converted, split="train"):
    return json.loads((converted / f"endovis18_coco_annotations_{split}.json").read_text())


@pytest.mark.parametrize("k", [10, 3, 1])
def test_opening_equals_rect_erode_dilate(converted, k):
    coco = _anns(converted)
    before = copy.deepcopy(coco)
    stats = {}
    out = OPEN.apply_morphological_closing_to_annotations(coco, kernel_size=k, on_device=False, stats=stats)
    assert out is coco
    lo, hi = -(k // 2), k - 1 - k // 2
    assert OPEN.opening_window(k) == (lo, hi)
    kept = []
    for a in before["annotations"]:
        m = rle.decode(a["segmentation"])
        o = rect_dilate(rect_erode(m, (lo, hi), (lo, hi)), (lo, hi), (lo, hi))
        if o.any():
            kept.append(dict(a, segmentation=rle.encode(o), area=int(o.sum())))  # bbox untouched
    assert coco["annotations"] == kept
    assert stats["removed"] == len(before["annotations"]) - len(kept) and stats["annotations"] == len(before["annotations"])
    if k == 1:
        assert coco == before  # the identity
    if k == 10:
        assert stats["removed"] >= 3  # the unlisted 6 x 5 block and the two thin bars
        assert not [a for a in coco["annotations"] if a["category_id"] == 9]
        assert any(a["area"] < b["area"] and a["bbox"] == b["bbox"]
                   for a in coco["annotations"] for b in before["annotations"] if a["id"] == b["id"])


def test_opening_quirks_and_limits(converted):
    coco = _anns(converted, "val")
    first = coco["annotations"][0]
    h, w, counts = rle.counts_of(first["segmentation"])
    forms = [dict(first, id=100, segmentation={"size": [h, w], "counts": counts}),     # uncompressed list
             dict(first, id=101, segmentation=repr(first["segmentation"])),            # the dict's repr
             dict(first, id=102, segmentation=None), {"id": 103, "image_id": 0}]       # passed through
    probe = {"images": coco["images"], "annotations": [copy.deepcopy(first)] + forms, "categories": coco["categories"]}
    OPEN.apply_morphological_closing_to_annotations(probe, kernel_size=10, on_device=False)
    got = probe["annotations"]
    assert got[1]["segmentation"] == got[0]["segmentation"] == got[2]["segmentation"]
    assert got[3]["segmentation"] is None and got[4] == {"id": 103, "image_id": 0}
    with pytest.raises(ValueError, match="67"):
        OPEN.apply_morphological_closing_to_annotations(_anns(converted), kernel_size=67, on_device=False)
    assert OPEN.opening_window(65) == (-32, 32)


def test_opening_window_is_what_cv2_wrote():
    """the reference's opened masks are fixed points of `dilate after the adjoint erosion` only for the
    dilation window the tool uses: O = dilate_w(Y) implies dilate_w(erode_-w(O)) == O"""
    lo, hi = OPEN.opening_window(10)
    assert (lo, hi) == (-5, 4)
    golden = json.load(open(os.path.join(GOLDEN, "rle_endovis18_sample.json")))
    assert len(golden["opened"]) == 24
    for a in golden["opened"]:
        m = rle.decode(a["segmentation"]).astype(bool)
        assert (rect_dilate(rect_erode(m, (-hi, -lo), (-hi, -lo)), (lo, hi), (lo, hi)) == m).all()
        assert int(m.sum()) == int(a["area"])


def test_keyframe_update_and_dry_run(converted, tmp_path):
    coco = _anns(converted)
    OPEN.apply_morphological_closing_to_annotations(coco, kernel_size=10, on_device=False)
    path = tmp_path / "opened.json"
    path.write_text(json.dumps(coco, indent=2))
    before = path.read_text()
    KEY.process_coco_file(path, backup=False, dry_run=True)
    assert path.read_text() == before and not (tmp_path / "opened.json.backup").exists()
    KEY.process_coco_file(path, backup=True)
    assert (tmp_path / "opened.json.backup").read_text() == before
    after = json.loads(path.read_text())
    flags = {i["id"]: i["is_det_keyframe"] for i in after["images"]}
    assert flags == {0: True, 1: True, 3: False, 4: False, 5: True}  # all background; only thin pieces
    assert after["annotations"] == coco["annotations"]
    again = KEY.update_is_det_keyframe(copy.deepcopy(after))
    assert again == after


def _run_module(name, *args):
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", name, *[str(a) for a in args]], env=env, capture_output=True,
                          text=True, timeout=300)


def test_the_three_commands_chain(tree, converted, tmp_path):
    root, _ = tree
    r = _run_module("sam2_video.data.convert_endovis_to_coco", "--source_dir", root, "--output_dir", tmp_path,
                    "--n_jobs", 2, "--host")
    assert r.returncode == 0, r.stderr
    for split in ("train", "val"):
        name = f"endovis18_coco_annotations_{split}.json"
        assert (tmp_path / name).read_text() == (converted / name).read_text()
    src, dst = tmp_path / "endovis18_coco_annotations_train.json", tmp_path / "train_opened.json"
    r = _run_module("sam2_video.data.apply_morphological_opening", src, dst, "--kernel-size", 10, "--host")
    assert r.returncode == 0, r.stderr
    want = _anns(converted)
    OPEN.apply_morphological_closing_to_annotations(want, kernel_size=10, on_device=False)
    assert dst.read_text() == json.dumps(want, indent=2)
    r = _run_module("sam2_video.data.update_is_det_keyframe", dst, "--no-backup")
    assert r.returncode == 0, r.stderr
    assert not (tmp_path / "train_opened.json.backup").exists()
    assert [i["is_det_keyframe"] for i in json.loads(dst.read_text())["images"]] == [True, True, False, False, True]
    from sam2_video.data.dataset import COCOImageDataset
    assert len(COCOImageDataset({"image_size": 64}, str(dst))) == 3


def test_converter_reproduces_the_reference_annotations(tmp_path):
    """three images of the reference's data/endovis18.json (pycocotools wrote it): label images painted from its
    masks convert back to its counts, areas and boxes"""
    fixture = json.load(open(os.path.join(GOLDEN, "dataprep_endovis18_images.json")))
    assert len(fixture["images"]) == 3 and len(fixture["annotations"]) == 12
    want = DC.paint_fixture(tmp_path / "src", fixture)
    conv = CONV.EndoVisToCOCOConverter(tmp_path / "src", tmp_path / "out", on_device=False)
    DC.check_fixture_output(conv.convert_split("val"), want)
