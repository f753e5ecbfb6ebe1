"""Dataset preparation on the device: s2h_label_hist and s2h_label_planes (csrc/dataprep.hip through ops.label_hist,
ops.label_planes and ops.mask_planes) against numpy on every case of dataprep_cases.py -- the ones
test_dataprep_host.py runs through the header on the host -- and the converter and the opening with on_device=True
against their host paths: the same JSON text, byte for byte."""
import copy
import json
import os

import numpy as np
import pytest
import torch

import dataprep_cases as DC
from sam2_video.data import apply_morphological_opening as OPEN
from sam2_video.data import convert_endovis_to_coco as CONV
from sam2_video.data import rle
from sam2_video.data import update_is_det_keyframe as KEY
from sam2_video.kernels import ops

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def cases():
    cs = DC.make_cases()
    return cs, [DC.reference(c) for c in cs]


def _run(c):
    labels = torch.from_numpy(c["labels"]).cuda()
    frame_off = torch.from_numpy(c["frame_off"]).cuda()
    plane_class = torch.from_numpy(c["plane_class"]).cuda()
    hist = ops.label_hist(labels)
    if c["plane_class"].size and (c["plane_class"] == -1).all():
        bits = ops.mask_planes(labels)
    else:
        bits = ops.label_planes(labels, frame_off, plane_class)
    return hist, bits


def test_kernels_equal_numpy(cases):
    cs, refs = cases
    for c, (want_hist, want_bits) in zip(cs, refs):
        hist, bits = _run(c)
        assert hist.dtype == torch.int32 and bits.dtype == torch.int64 and hist.is_cuda and bits.is_cuda
        assert torch.equal(hist.cpu(), torch.from_numpy(want_hist)), c["name"]
        assert torch.equal(bits.cpu(), torch.from_numpy(want_bits)), c["name"]


def test_kernels_on_a_side_stream_and_twice_in_a_row(cases):
    cs, refs = cases
    side = torch.cuda.Stream()
    for c, (want_hist, want_bits) in zip(cs, refs):
        first = _run(c)
        second = _run(c)
        assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1]), c["name"]
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            hist, bits = _run(c)
        side.synchronize()
        assert torch.equal(hist.cpu(), torch.from_numpy(want_hist)), c["name"]
        assert torch.equal(bits.cpu(), torch.from_numpy(want_bits)), c["name"]


def test_launcher_argument_checks():
    from sam2_video.kernels._lib import HipKernelError
    labels = torch.zeros(1, 4, 4, dtype=torch.uint8, device="cuda")
    empty = ops.label_planes(labels, torch.zeros(2, dtype=torch.int32, device="cuda"),
                             torch.zeros(0, dtype=torch.int32, device="cuda"))
    assert tuple(empty.shape) == (0, 1)  # P == 0: no launch
    big = torch.zeros(1, 4097, 4096, dtype=torch.uint8, device="cuda")  # H W > 2^24
    with pytest.raises(HipKernelError):
        ops.label_hist(big)
    with pytest.raises(HipKernelError):
        ops.mask_planes(big)


def test_real_size_planes_and_header_area():
    """1024 x 1280, two frames, four classes: exactly 64 KB of tile per band, 20 bands; the histogram equals the
    area s2h_rle_transitions reads from the planes"""
    H, W = 1024, 1280
    labels = np.zeros((2, H, W), np.uint8)
    for f in range(2):
        for c, (y0, x0, y1, x1) in zip((1, 2, 5, 255), ((0, 0, 500, 333), (17, 300, 1024, 700), (400, 650, 901, 1280),
                                                        (950, 1, 1023, 1279))):
            labels[f, y0:y1, x0 + 13 * f:x1] = c
        labels[f, ::7, 3::11] = 0
    case = DC.make_case("real", labels)
    assert case["plane_class"].tolist() == [1, 2, 5, 255] * 2
    want_hist, want_bits = DC.reference(case)
    hist, bits = _run(case)
    assert torch.equal(hist.cpu(), torch.from_numpy(want_hist))
    assert torch.equal(bits.cpu(), torch.from_numpy(want_bits))
    hdr, _ = ops.rle_transitions(bits, H, W, capacity=4096)
    hdr = hdr.cpu().numpy()
    for p, c in enumerate(case["plane_class"]):
        assert hdr[p, 2] == want_hist[p // 4, c]


# ------------------------------------------------------------------------------ the tools
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = tmp_path_factory.mktemp("endovis") / "src"
    t = DC.build_tree(root)
    out = tmp_path_factory.mktemp("coco_host")
    with pytest.warns(UserWarning):
        CONV.EndoVisToCOCOConverter(root, out, on_device=False).convert_dataset()
    return root, t, out


@pytest.mark.parametrize("chunks", [{}, {"frames_per_call": 1, "planes_per_call": 2}])
def test_converter_on_device_writes_the_same_text(tree, tmp_path, chunks):
    root, _, host = tree
    conv = CONV.EndoVisToCOCOConverter(root, tmp_path, on_device=True, **chunks)
    with pytest.warns(UserWarning):
        conv.convert_dataset()
    for split in ("train", "val"):
        name = f"endovis18_coco_annotations_{split}.json"
        assert (tmp_path / name).read_text() == (host / name).read_text()
    assert conv.stats["bytes_up"] > 0 and conv.stats["bytes_down"] > 0
    label_path = root / "train" / "annotations" / "seq_1_frame001.png"
    assert conv.process_annotation_mask(label_path, 7) == conv.process_annotation_mask(label_path, 7, on_device=False)


@pytest.mark.parametrize("k,per_call", [(10, None), (10, 2), (3, None), (1, None)])
def test_opening_on_device_writes_the_same_text(tree, k, per_call):
    _, _, host = tree
    coco = json.loads((host / "endovis18_coco_annotations_train.json").read_text())
    want, got = copy.deepcopy(coco), copy.deepcopy(coco)
    OPEN.apply_morphological_closing_to_annotations(want, kernel_size=k, on_device=False)
    stats = {}
    OPEN.apply_morphological_closing_to_annotations(got, kernel_size=k, on_device=True, anns_per_call=per_call,
                                                    stats=stats)
    assert json.dumps(got, indent=2) == json.dumps(want, indent=2)
    assert stats["removed"] == len(coco["annotations"]) - len(got["annotations"])
    with pytest.raises(ValueError):
        OPEN.apply_morphological_closing_to_annotations(copy.deepcopy(coco), kernel_size=67, on_device=True)


def test_fixture_through_the_device_path(tmp_path):
    """the three reference images at their real 1024 x 1280: what pycocotools wrote comes back from the kernels"""
    fixture = json.load(open(os.path.join(GOLDEN, "dataprep_endovis18_images.json")))
    want = DC.paint_fixture(tmp_path / "src", fixture)
    conv = CONV.EndoVisToCOCOConverter(tmp_path / "src", tmp_path / "out", on_device=True)
    DC.check_fixture_output(conv.convert_split("val"), want)


def test_opening_moves_no_mask_across_the_bus():
    golden = json.load(open(os.path.join(GOLDEN, "rle_endovis18_sample.json")))["original"]
    assert len(golden) == 24
    coco = {"images": [], "categories": [],
            "annotations": [{"id": i, "image_id": 0, "category_id": 0, "segmentation": a["segmentation"],
                             "area": int(a["area"]), "bbox": a["bbox"]} for i, a in enumerate(golden)]}
    want = copy.deepcopy(coco)
    stats = {}
    OPEN.apply_morphological_closing_to_annotations(coco, kernel_size=10, on_device=True, stats=stats)
    h, w = rle._as_rle(golden[0]["segmentation"])["size"]
    assert stats["annotations"] == 24
    assert stats["bytes_up"] > 0 and stats["bytes_down"] > 0
    assert stats["bytes_up"] + stats["bytes_down"] < 24 * h * w  # below one H x W byte mask per annotation
    OPEN.apply_morphological_closing_to_annotations(want, kernel_size=10, on_device=False)
    assert coco == want


def test_the_chain_ends_in_a_file_the_dataset_loads(tree, tmp_path):
    root, _, _ = tree
    with pytest.warns(UserWarning):
        CONV.EndoVisToCOCOConverter(root, tmp_path, on_device=True).convert_dataset()
    src, dst = tmp_path / "endovis18_coco_annotations_train.json", tmp_path / "train_opened.json"
    OPEN.process_coco_file(src, dst, kernel_size=10, on_device=True)
    KEY.process_coco_file(dst, backup=False)
    from sam2_video.data.dataset import COCOImageDataset
    data = json.loads(dst.read_text())
    keyframes = [i for i in data["images"] if i["is_det_keyframe"]]
    assert len(keyframes) == 3 < len(data["images"])
    assert len(COCOImageDataset({"image_size": 64}, str(dst))) == len(keyframes)
