"""The offline scoring's pair counts on the device (csrc/rle.hip s2h_rle_pair_counts through ops.rle_pair_counts):
the cases of pair_counts_cases.py -- the ones test_pair_counts_host.py runs through the header on the host --
against numpy decode / OR / sum, equal integers; and eval(score_on_device=True) against eval(score_on_device=False)
on a small synthetic COCO pair (two mask sizes, several annotations per category, one-sided categories, an image
without annotations, a non-keyframe image, remove_background)."""
import json
import math
import pickle

import numpy as np
import pytest
import torch

import pair_counts_cases as PC
from sam2_video.data import rle
from sam2_video.kernels import ops

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    cs = PC.make_cases()
    return cs, [PC.reference(c) for c in cs]


def test_kernel_counts_equal_numpy(cases):
    cs, refs = cases
    for c, want in zip(cs, refs):
        got = ops.rle_pair_counts(c["dt"], c["gt"], c["H"], c["W"])
        assert got.dtype == torch.int64 and got.is_cuda and tuple(got.shape) == want.shape
        g = got.cpu().numpy()
        assert (g == want).all(), (c["name"], g[(g != want).any(axis=1)][:3], want[(g != want).any(axis=1)][:3])


def test_launcher_argument_checks():
    assert tuple(ops.rle_pair_counts([], [], 4, 4).shape) == (0, 4)
    with pytest.raises(ValueError):
        ops.rle_pair_counts([[]], [], 4, 4)
    with pytest.raises(ValueError):  # counts that do not cover the image
        ops.rle_pair_counts([[[3, 4]]], [[]], 4, 4)
    with pytest.raises(ValueError):
        ops.rle_pair_counts([[[16]] * (ops.PC_MAX_GROUP_ANNS + 1)], [[]], 4, 4)


def _coco_pair(tmp_path):
    rng = np.random.default_rng(11)
    images, gts, dts = [], [], []
    sizes = [(37, 53), (37, 53), (64, 40), (37, 53), (64, 40)]
    for i, (h, w) in enumerate(sizes):
        image_id = i + 1
        images.append({"id": image_id, "video_id": "v%d" % (i // 3), "order_in_video": i % 3, "height": h, "width": w,
                       "is_det_keyframe": i != 1})
        if i == 3:
            continue  # an image without any annotation
        for cat in (0, 1, 2, 3):
            n_gt = int(rng.integers(0, 3)) if cat != 3 else 0  # category 3 is never in the ground truth
            n_dt = int(rng.integers(0, 3)) if cat != 2 else 0  # category 2 is never predicted
            for side, n in ((gts, n_gt), (dts, n_dt)):
                for _ in range(n):
                    m = PC._blob(rng, h, w)
                    side.append({"id": len(side) + 1, "image_id": image_id, "category_id": cat,
                                 "segmentation": rle.encode(m), "area": int(m.sum()), "iscrowd": 0})
    coco = {"images": images, "annotations": gts, "categories": [{"id": c, "name": str(c)} for c in (0, 1, 2, 3)]}
    coco_path, predict_path = tmp_path / "coco.json", tmp_path / "predict.json"
    coco_path.write_text(json.dumps(coco))
    predict_path.write_text(json.dumps(dts))
    assert len(gts) > 6 and len(dts) > 6
    return str(coco_path), str(predict_path)


def _same(a, b, path="result"):
    if isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b), path
        for k in a:
            _same(a[k], b[k], f"{path}[{k!r}]")
    elif isinstance(a, (list, tuple)):
        assert type(a) is type(b) and len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{path}[{i}]")
    elif isinstance(a, float) and math.isnan(a):
        assert isinstance(b, float) and math.isnan(b), path
    else:
        assert type(a) is type(b) and a == b, (path, a, b)


@pytest.mark.parametrize("remove_background", [False, True])
def test_eval_on_device_equals_eval_on_host(tmp_path, remove_background):
    from sam2_video.eval import eval as E
    coco_path, predict_path = _coco_pair(tmp_path)
    res = {}
    for on_device in (True, False):
        out = tmp_path / ("dev" if on_device else "host")
        res[on_device] = E.eval(predict_path, coco_path, str(out), remove_background=remove_background,
                                score_on_device=on_device)
        with open(out / "eval.pkl", "rb") as f:
            _same(pickle.load(f), res[on_device])
    _same(res[True], res[False])
    _same(E.eval(predict_path, coco_path, str(tmp_path / "default"), remove_background=remove_background), res[False])
    r = res[False]
    assert list(r["cat_scores"]) == ([1, 2, 3] if remove_background else [0, 1, 2, 3])
    assert sum(len(v["frames"]) for v in r["videos"]) == 4  # the non-keyframe image is not scored
    assert all(math.isfinite(r["avg_scores"][k]) for k in E.KEYS) and r["avg_scores"]["iou"] > 0
    assert r["cat_scores"][2]["iou"] == 0.0 and r["cat_scores"][3]["dice"] == 0.0  # one-sided categories
