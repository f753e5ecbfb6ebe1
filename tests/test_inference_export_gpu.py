"""The evaluation surface end to end (sam2_video/eval/inference.py): Hiera-T at 256^2, bf16, a clip of five
frames of (S + 16) x (S + 32) pixels, three objects with ids 1, 2 and 1001 and mod = 1000 (1 and 1001 merge
into category 1), prompted by a click, a box and a mask on the middle frame.  The device export
(propagate_in_video_export -> csrc/rle.hip) against the reference's host loop (export_on_device=False): the two
predict.json files, the tracking state, the probability dumps and the scores the file earns."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from step_harness import build_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

pytestmark = pytest.mark.gpu

S, T, MOD = 256, 5, 1000
H, W = S + 16, S + 32
START, PROMPT = 1, 3  # the clip is frames 1..5 of a video of 7; prompts on order_in_video 3 (the clip's middle)
IDS = [1, 2, 1001]


def _frames():
    return [{"id": 100 + t, "video_id": "v0", "order_in_video": t, "height": H, "width": W, "path": f"{t}.jpg"}
            for t in range(T + 2)]


def _prompts():
    from sam2_video.eval.utils import ClipRange, PromptInfo, PromptObj
    mask = np.zeros((H, W), bool)
    mask[40:110, 60:170] = True
    clip = ClipRange(START, START + T - 1)
    objs = [("point", PromptObj(mask=None, bbox=None, points=[[100.0, 90.0]], obj_id=1, pos_or_neg_label=[1])),
            ("box", PromptObj(mask=None, bbox=[10.0, 20.0, 130.0, 150.0], points=None, obj_id=2, pos_or_neg_label=None)),
            ("mask", PromptObj(mask=mask, bbox=None, points=None, obj_id=1001, pos_or_neg_label=None))]
    return clip, [PromptInfo([o], PROMPT, kind, "v0", f"{PROMPT}.jpg", clip) for kind, o in objs]


def _run(model, video, out_dir, on_device, non_overlap, probs=False):
    """one clip through process_video_clip + save_as_coco_format -> everything the tests look at"""
    from sam2_video.eval import inference as I
    from sam2_video.predictor import SAM2VideoPredictor
    pred = SAM2VideoPredictor(model, fill_hole_area=8, non_overlap_masks=non_overlap)
    seen = {"state": None, "logits": {}, "merged": {}}
    real_init, real_prop, real_exp = pred.init_state, pred.propagate_in_video, pred.propagate_in_video_export

    def init_state(*a, **k):
        seen["state"] = real_init(*a, **k)
        return seen["state"]

    def propagate_in_video(state, *a, **k):  # keeps the host path's video-res logits (the later pass wins)
        for t, ids, logits in real_prop(state, *a, **k):
            seen["logits"][t + START] = logits.clone()
            yield t, ids, logits

    def propagate_in_video_export(state, *a, **k):
        for t, ids, merged in real_exp(state, *a, **k):
            seen["merged"][t + START] = (bool(k.get("reverse", False)), merged)
            yield t, ids, merged

    pred.init_state, pred.propagate_in_video = init_state, propagate_in_video
    pred.propagate_in_video_export = propagate_in_video_export
    clip, prompts = _prompts()
    frames = _frames()
    probs_dir = os.path.join(out_dir, "probs") if probs else None
    try:
        segs = I.process_video_clip(pred, frames, prompts, clip, probs_out_dir=probs_dir, video=video, mod=MOD,
                                    export_on_device=on_device)
    finally:  # the spies close over the predictor: take them off again, so no reference cycle is left behind
        del pred.init_state, pred.propagate_in_video, pred.propagate_in_video_export
    clip_frames = frames[clip.start_idx:clip.end_idx + 1]
    predict_path, prompt_path = I.save_as_coco_format({"v0": segs}, {"v0": clip_frames}, MOD, out_dir,
                                                      prompt_info=prompts)
    assert os.path.basename(predict_path) == "predict.json" and os.path.exists(prompt_path)
    return {"segs": segs, "json": json.load(open(predict_path)), "text": open(predict_path).read(),
            "state": seen["state"], "logits": seen["logits"], "merged": seen["merged"], "probs_dir": probs_dir}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    model = build_model("tiny", S, [], "point", dtype="bf16", seed=3)
    video = (torch.rand(T, H, W, 3, generator=torch.Generator().manual_seed(0)) * 255).to(torch.uint8).numpy()
    out = {}
    for non_overlap in (False, True):
        for on_device in (True, False):
            d = str(tmp_path_factory.mktemp(f"eval_{int(non_overlap)}_{int(on_device)}"))
            out[(non_overlap, on_device)] = _run(model, video, d, on_device, non_overlap, probs=not non_overlap)
    return out


@pytest.mark.parametrize("non_overlap", [False, True], ids=["overlap", "non_overlap"])
def test_predict_json_equals_the_host_path(runs, non_overlap):
    dev, host = runs[(non_overlap, True)], runs[(non_overlap, False)]
    a, b = dev["json"], host["json"]
    assert len(a) == len(b) > 0
    assert dev["text"].startswith("[\n    {\n        \"image_id\"")  # indent=4
    for x, y in zip(a, b):  # the same annotations in the same order
        assert list(x) == list(y) == ["image_id", "category_id", "segmentation", "bbox", "iscrowd", "score"]
        for k in ("image_id", "category_id", "segmentation", "bbox", "iscrowd"):
            assert x[k] == y[k], (k, x["image_id"], x["category_id"])
        assert x["segmentation"]["size"] == [H, W] and isinstance(x["segmentation"]["counts"], str)
        assert abs(x["score"] - y["score"]) <= 1e-5
    # every frame of the clip appears, with categories 1 (objects 1 and 1001) and 2 at most
    assert sorted({x["image_id"] for x in a}) == [100 + t for t in range(START, START + T)]
    assert {x["category_id"] for x in a} <= {1, 2}
    assert sorted(dev["segs"]) == sorted(host["segs"]) == list(range(START, START + T))
    # the score of every annotation of a frame is the one of the frame's LAST object (1001), in both files
    for x, y in zip(a, b):
        order = x["image_id"] - 100
        assert x["score"] == dev["segs"][order]["scores"][1001]
        assert y["score"] == host["segs"][order][1001]["score"]
        assert list(dev["segs"][order]["scores"]) == IDS == list(host["segs"][order])
    # per-object scores, not only the last one's
    for order in dev["segs"]:
        for i in IDS:
            assert abs(dev["segs"][order]["scores"][i] - host["segs"][order][i]["score"]) <= 1e-5
    # the prompt frame carries the forward pass's result (the reverse pass visited it first)
    reverse, merged = dev["merged"][PROMPT]
    assert reverse is False and merged.result() is dev["segs"][PROMPT]
    assert dev["merged"][START][0] is True and dev["merged"][START + T - 1][0] is False
    if non_overlap:  # the constraint really changed something
        assert runs[(False, True)]["json"] != a


@pytest.mark.parametrize("non_overlap", [False, True], ids=["overlap", "non_overlap"])
def test_export_tracks_exactly_like_propagate_in_video(runs, non_overlap):
    sd, sh = runs[(non_overlap, True)]["state"], runs[(non_overlap, False)]["state"]
    assert sd is not sh and sd["obj_ids"] == sh["obj_ids"] == IDS
    assert sd["frames_tracked_per_obj"] == sh["frames_tracked_per_obj"]
    n = 0
    for i in range(len(IDS)):
        for key in ("cond_frame_outputs", "non_cond_frame_outputs"):
            assert sorted(sd["output_dict_per_obj"][i][key]) == sorted(sh["output_dict_per_obj"][i][key])
            for t, e in sd["output_dict_per_obj"][i][key].items():
                f = sh["output_dict_per_obj"][i][key][t]
                for name in ("pred_masks", "obj_ptr", "maskmem_features", "object_score_logits"):
                    assert e[name] is not None and torch.equal(e[name], f[name]), (i, key, t, name)  # atol = 0
                    n += 1
    assert n == len(IDS) * T * 4


def test_staging_blocks_are_reused(runs):
    """ten tracked frames with one in flight: the state's pool ends with two pinned blocks, not ten"""
    for non_overlap in (False, True):
        pool = runs[(non_overlap, True)]["state"]["export_staging"]
        slots = [slot for free in pool._free.values() for slot in free]
        assert len(slots) == 2 and all(t.is_pinned() for t, _ in slots)
        assert not any(free for free in runs[(non_overlap, False)]["state"]["export_staging"]._free.values())


def test_probability_dumps(runs):
    dev, host = runs[(False, True)], runs[(False, False)]
    for run in (dev, host):
        names = sorted(os.listdir(run["probs_dir"]))
        assert names == [f"{100 + t}.npz" for t in range(START, START + T)]
    for t in range(START, START + T):
        z = np.load(os.path.join(dev["probs_dir"], f"{100 + t}.npz"))
        zh = np.load(os.path.join(host["probs_dir"], f"{100 + t}.npz"))
        assert sorted(z.files) == sorted(["probs", "obj_ids", "image_id", "video_id", "order_in_video", "height",
                                          "width"])
        assert z["probs"].dtype == np.float16 and z["probs"].shape == (len(IDS), H, W)
        assert z["obj_ids"].dtype == np.int64 and list(z["obj_ids"]) == IDS
        assert z["image_id"].dtype == np.int64 and int(z["image_id"]) == 100 + t
        assert str(z["video_id"]) == "v0" and z["order_in_video"].dtype == np.int64 and int(z["order_in_video"]) == t
        assert z["height"].dtype == np.int32 and z["width"].dtype == np.int32
        assert (int(z["height"]), int(z["width"])) == (H, W)
        assert np.array_equal(z["probs"], zh["probs"])
        # the dump is the float16 sigmoid of the very logits the export thresholds: rounded to nearest, except
        # that a positive logit whose sigmoid rounds to exactly one half is stored one float16 step above it
        logits = host["logits"][t][:, 0]
        nearest = torch.sigmoid(logits).cpu().numpy().astype(np.float16)
        lifted = (nearest == np.float16(0.5)) & (logits > 0).cpu().numpy()
        above_half = np.float16(0.5 + 2.0 ** -11)
        assert above_half > np.float16(0.5) and np.nextafter(above_half, np.float16(0)) == np.float16(0.5)
        assert np.array_equal(z["probs"], np.where(lifted, above_half, nearest))
        assert lifted.any()  # (on this clip the rule is exercised: some logits lie in (0, 2^-10])
        # so every stored value stays on its logit's side of one half
        assert np.array_equal(z["probs"] > 0.5, (logits > 0).cpu().numpy())


def test_probs_above_half_agree_with_the_exported_masks(runs):
    """`probs > 0.5` of the dumps against the exported masks after the same category OR, on every pixel.

    With sigmoid(v) rounded to the nearest float16, 180 pixels of this clip differed (2 to 29 of 78336 per
    frame and category): float16 has no value between 0.5 and 0.50049, so a logit 0 < v <= 2^-10 = 9.766e-4 was
    stored as exactly 0.5 and `> 0.5` dropped a pixel that `v > 0` -- the threshold of predict.json, in the
    reference and in the export -- keeps.  The dump now stores those pixels one float16 step above one half
    (eval/inference.py, _maybe_write_probs).  Should pixels differ, the test prints per frame and category how
    many of them are exported, stored as exactly 0.5 and have a positive logit, and the largest logit."""
    from sam2_video.data import rle
    dev, host = runs[(False, True)], runs[(False, False)]
    by_image = {}
    for x in dev["json"]:
        by_image.setdefault(x["image_id"], {})[x["category_id"]] = rle.decode(x["segmentation"]).astype(bool)
    bad = 0
    for t in range(START, START + T):
        z = np.load(os.path.join(dev["probs_dir"], f"{100 + t}.npz"))
        logits = host["logits"][t][:, 0].cpu().numpy()
        for cat in (1, 2):
            ks = [k for k, i in enumerate(IDS) if i % MOD == cat]
            want = np.logical_or.reduce([z["probs"][k] > 0.5 for k in ks], axis=0)
            got = by_image.get(100 + t, {}).get(cat, np.zeros((H, W), bool))
            diff = want != got
            if diff.any():
                vmax = np.max([logits[k] for k in ks], axis=0)
                half = np.logical_or.reduce([(z["probs"][k] == 0.5) & (logits[k] > 0) for k in ks], axis=0)
                print(f"frame {t} category {cat}: {int(diff.sum())} of {H * W} pixels differ, "
                      f"{int((diff & half & got).sum())} of them exported, float16 0.5 and logit > 0; "
                      f"largest logit among them {float(vmax[diff].max()):.3e}")
            bad += int(diff.sum())
    assert bad == 0, f"{bad} pixels differ"


def test_the_file_scores_what_the_in_loop_validation_scores(runs):
    """decode the device path's RLEs -> oracle image_scores against a synthetic ground truth; the host path's
    category-merged video-res logits -> frame_counts + image_scores_from_counts: the same numbers"""
    import eval_oracle as EO
    from sam2_video.data import rle
    from sam2_video.eval import eval as E
    dev, host = runs[(False, True)], runs[(False, False)]
    cats = [1, 2, 3]  # (3: never predicted; with an empty ground truth it reads NaN on both sides)
    gt = np.zeros((len(cats), H, W), bool)
    gt[0, 30:120, 50:180] = True
    gt[1, 10:160, 5:140] = True
    for t in range(START, START + T):
        pred = np.zeros((len(cats), H, W), bool)
        for x in dev["json"]:
            if x["image_id"] == 100 + t:
                pred[cats.index(x["category_id"])] = rle.decode(x["segmentation"]).astype(bool)
        want = EO.image_scores(pred, gt, cats)
        logits = host["logits"][t]  # [N, 1, H, W]
        merged = torch.stack([torch.stack([logits[k] for k, i in enumerate(IDS) if i % MOD == c]).amax(dim=0)
                              if any(i % MOD == c for i in IDS) else torch.full_like(logits[0], -1.0) for c in cats])
        counts = E.frame_counts(merged.contiguous(), torch.from_numpy(gt).cuda()).cpu().numpy()
        got = E.image_scores_from_counts(counts, H * W, cats)
        for c in cats:
            for k in E.KEYS:
                a, b = want["cat_scores"][c][k], got["cat_scores"][c][k]
                assert (np.isnan(a) and np.isnan(b)) or abs(a - b) <= 1e-12, (t, c, k, a, b)
    assert np.isnan(want["cat_scores"][3]["iou"]) and want["cat_scores"][1]["iou"] > 0
