"""Threshold tuning end to end on the clip of tests/test_inference_export_gpu.py (Hiera-T at 256^2, five frames of
272 x 288, objects 1, 2 and 1001 with mod = 1000): the device sweep (predict_on_video(sweep=...)) against counts
taken from propagate_in_video's video-resolution logits and against the reference's way (probs_out_dir + the host
grid_search), and the export at a threshold (threshold= + save_thresholded_predict) against rle.encode of the
logits and export_predict over the dump."""
import json
import os

import numpy as np
import pytest
import torch

import sweep_ref as R
from step_harness import build_model
from test_inference_export_gpu import H, IDS, MOD, PROMPT, S, START, T, W, _frames, _prompts

pytestmark = pytest.mark.gpu

CAT_IDS = [1, 2]            # first-seen order of IDS % MOD
CATS = [[0, 2], [1]]        # their objects
NO_GT = 100 + START + 1     # the frame without annotations


def _coco():
    from sam2_video.data import rle
    anns = []
    for t in range(START, START + T):
        image_id = 100 + t
        if image_id == NO_GT:
            continue
        a, b = np.zeros((H, W), bool), np.zeros((H, W), bool)
        a[30 + t:120 + t, 50:180] = True
        b[10:160, 5 + 2 * t:140] = True
        anns += [{"image_id": image_id, "category_id": 1, "segmentation": rle.encode(a)},
                 {"image_id": image_id, "category_id": 2, "segmentation": rle.encode(b)}]
    c = np.zeros((H, W), bool)
    c[200:230, 200:260] = True
    anns.append({"image_id": 100 + PROMPT, "category_id": 3, "segmentation": rle.encode(c)})  # never predicted
    for i, a in enumerate(anns):
        a["id"] = i + 1
    return {"annotations": anns}


def _run(model, video, on_device, probs_dir=None, **kw):
    from sam2_video.eval import inference as I
    from sam2_video.predictor import SAM2VideoPredictor
    pred = SAM2VideoPredictor(model, fill_hole_area=8)
    seen = {"state": None, "first": {}, "last": {}, "merged": {}}
    real_init, real_prop, real_exp = pred.init_state, pred.propagate_in_video, pred.propagate_in_video_export

    def init_state(*a, **k):
        seen["state"] = real_init(*a, **k)
        return seen["state"]

    def propagate_in_video(state, *a, **k):
        for t, ids, logits in real_prop(state, *a, **k):
            seen["first"].setdefault(t + START, logits[:, 0].cpu().numpy())
            seen["last"][t + START] = logits[:, 0].cpu().numpy()
            yield t, ids, logits

    def propagate_in_video_export(state, *a, **k):
        for t, ids, merged in real_exp(state, *a, **k):
            seen["merged"].setdefault(t + START, []).append(merged)
            yield t, ids, merged

    pred.init_state, pred.propagate_in_video = init_state, propagate_in_video
    pred.propagate_in_video_export = propagate_in_video_export
    clip, prompts = _prompts()
    try:
        seen["segs"] = I.process_video_clip(pred, _frames(), prompts, clip, probs_out_dir=probs_dir, video=video,
                                            mod=MOD, export_on_device=on_device, **kw)
    finally:
        del pred.init_state, pred.propagate_in_video, pred.propagate_in_video_export
    return seen


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    from sam2_video.eval import tune_threshold as TT
    from sam2_video.eval.export_predict_from_probs import export_predict
    model = build_model("tiny", S, [], "point", dtype="bf16", seed=3)
    video = (torch.rand(T, H, W, 3, generator=torch.Generator().manual_seed(0)) * 255).to(torch.uint8).numpy()
    d = tmp_path_factory.mktemp("tune")
    probs_dir = str(d / "probs")
    coco = _coco()
    out = {"coco": coco, "dir": str(d), "probs_dir": probs_dir}
    out["host"] = _run(model, video, False, probs_dir)
    TT.write_meta(probs_dir, MOD)
    out["grid"] = TT.grid_search(probs_dir, coco)
    out["plain"] = _run(model, video, True)
    acc = TT.SweepAccumulator(TT.threshold_grid(), coco, MOD)
    out["swept"], out["acc"] = _run(model, video, True, sweep=acc), acc
    out["thr"] = {}
    for t in dict.fromkeys([acc.result()[0], 0.35]):
        out["thr"][t] = (_run(model, video, True, threshold=t), export_predict(probs_dir, t, str(d / f"host_{t}.json")))
    return out


def _gt(coco, image_id):
    from sam2_video.data import rle
    gt = np.zeros((len(CAT_IDS), H, W), bool)
    for a in coco["annotations"]:
        if a["image_id"] == image_id and a["category_id"] in CAT_IDS:
            gt[CAT_IDS.index(a["category_id"])] |= rle.decode(a["segmentation"]).astype(bool)
    return gt


def test_frame_counts_equal_the_logits_counts(runs):
    """every frame's histogram is the numpy histogram of propagate_in_video's logits of the FIRST visit (the
    prompt frame is visited by both passes) against the ground truth; then the curve from those counts"""
    from sam2_video.eval import tune_threshold as TT
    acc, host = runs["acc"], runs["host"]
    assert sorted(acc.frames) == [100 + t for t in range(START, START + T)]
    assert len(runs["swept"]["merged"][PROMPT]) == 2 and sorted(host["first"]) == sorted(host["last"])
    again = TT.SweepAccumulator(acc.thresholds, runs["coco"], MOD)
    for t in range(START, START + T):
        want = R.np_hist(host["first"][t], CATS, acc.cuts, _gt(runs["coco"], 100 + t))
        assert np.array_equal(acc.frames[100 + t], want), t
        assert np.all(want.sum(axis=(1, 2)) == H * W)
        assert (want[:, 1].sum() == 0) == (100 + t == NO_GT)
        seg = runs["swept"]["segs"][t]
        assert seg["cat_ids"] == CAT_IDS and seg["sweep"].dtype == np.int32 and seg["sweep"].shape == (2, 2, 14)
    # summed in the accumulator's own order (the reverse pass first), the curve is the same to the last bit
    for image_id in acc.frames:
        t = image_id - 100
        again.add_frame(image_id, IDS, CAT_IDS, R.np_hist(host["first"][t], CATS, acc.cuts, _gt(runs["coco"], image_id)))
    assert again.result() == acc.result()
    assert list(acc.count) == [2 * T + 1] * 13  # categories 1 and 2 per frame, category 3 once (Dice 0)


def test_curve_against_the_host_grid_search(runs):
    """the reference's way: the float16 dump and grid_search over it.  Per threshold the curves differ by at most
    what the ambiguous pixels (|sigmoid(v) - mid| <= 2^-22) can move the mean Dice: one pixel moves one
    category's 2 I / (P + G) by at most 2 / (P + G - A)"""
    acc, host = runs["acc"], runs["host"]
    got, want = acc.result(), runs["grid"]
    amb = sum(R.ambiguous(host["first"][t], acc.thresholds).reshape(13, -1).sum(axis=1)
              for t in range(START, START + T))
    size = np.full(13, np.inf)
    for hist in acc.frames.values():
        pred = np.cumsum(hist.sum(axis=1)[:, ::-1], axis=1)[:, ::-1][:, 1:]  # [ncat, K]
        size = np.minimum(size, (pred + hist[:, 1].sum(axis=1, keepdims=True)).min(axis=0))
    exact = True
    for k, ((t, a), (t2, b)) in enumerate(zip(got[2], want[2])):
        bound = 2.0 * amb[k] / max(1.0, size[k] - amb[k]) / acc.count[k] + 1e-12
        print(f"threshold {t}: {int(amb[k])} ambiguous pixels, device {a:.12f} host {b:.12f} "
              f"difference {abs(a - b):.3e} (bound {bound:.3e})")
        assert t == t2 and abs(a - b) <= bound
        exact = exact and amb[k] == 0
    if exact:
        assert got[0] == want[0]
    assert len(got[2]) == 13 and 0.0 < got[1] < 1.0


@pytest.mark.parametrize("which", ["tuned", "0.35"])
def test_predict_at_a_threshold(runs, which):
    from sam2_video.data import rle
    from sam2_video.eval import inference as I
    from sam2_video.eval import tune_threshold as TT
    from sam2_video.eval.utils import mask_to_bbox
    t = runs["acc"].result()[0] if which == "tuned" else 0.35
    run, host_path = runs["thr"][t]
    clip_frames = _frames()[START:START + T]
    path = I.save_thresholded_predict({"v0": run["segs"]}, {"v0": clip_frames}, t,
                                      os.path.join(runs["dir"], f"dev_{which}.json"))
    text = open(path).read()
    assert text.startswith("[\n  {\n    \"image_id\"")  # indent=2
    anns = {(a["image_id"], a["category_id"]): a for a in json.loads(text)}
    host = {(a["image_id"], a["category_id"]): a for a in json.load(open(host_path))}
    cut = TT.logit_cuts([t])[0]
    want = {}
    for order in range(START, START + T):
        v = runs["host"]["last"][order]  # (the forward pass's result stands for the prompt frame)
        for cat, objs in zip(CAT_IDS, CATS):
            m = np.logical_or.reduce([v[o] >= cut for o in objs], axis=0)
            if m.any():
                want[(100 + order, cat)] = m
    assert sorted(anns) == sorted(want) and len(want) > T
    for key, m in want.items():
        a = anns[key]
        assert list(a) == ["image_id", "category_id", "segmentation", "bbox", "iscrowd", "score"]
        assert a["segmentation"] == rle.encode(m) and a["bbox"] == mask_to_bbox(m) and a["iscrowd"] == 0
        if key in host:  # the dump keeps the FIRST visit of the prompt frame, the export the last: same logits
            b = host[key]
            step = float(np.spacing(np.float16(max(a["score"], b["score"]))))
            assert abs(a["score"] - b["score"]) <= step, (key, a["score"], b["score"])
            amb = R.ambiguous(runs["host"]["last"][key[0] - 100], [t]).any()
            if not amb:
                assert a["segmentation"] == b["segmentation"] and a["bbox"] == b["bbox"]
    assert sorted(host) == sorted(anns)
    # the default name
    cwd = os.getcwd()
    os.chdir(runs["dir"])
    try:
        assert I.save_thresholded_predict({"v0": run["segs"]}, {"v0": clip_frames}, t) == f"predict_t{t:.2f}.json"
        assert json.load(open(f"predict_t{t:.2f}.json")) == json.loads(text)
    finally:
        os.chdir(cwd)
    with pytest.raises(ValueError):
        I.save_thresholded_predict({"v0": runs["plain"]["segs"]}, {"v0": clip_frames}, t, os.path.join(runs["dir"], "x"))


def test_the_sweep_rides_in_the_same_copy(runs):
    """bytes per frame: the plain export's plus ncat * 2 * (K + 1) * 4 exactly; the same two staging blocks; and
    the tracking state after a swept run is the plain run's, bit for bit"""
    plain, swept = runs["plain"], runs["swept"]
    n = 0
    for t in range(START, START + T):
        for a, b in zip(plain["merged"][t], swept["merged"][t]):
            assert b.bytes_copied - a.bytes_copied == len(CAT_IDS) * 2 * 14 * 4
            n += 1
    assert n == T + 1
    for run in (plain, swept, *[r for r, _ in runs["thr"].values()]):
        slots = [slot for free in run["state"]["export_staging"]._free.values() for slot in free]
        assert len(slots) == 2 and all(x.is_pinned() for x, _ in slots)
    sd, sh = swept["state"], plain["state"]
    assert sd is not sh and sd["obj_ids"] == sh["obj_ids"] == IDS
    n = 0
    for i in range(len(IDS)):
        for key in ("cond_frame_outputs", "non_cond_frame_outputs"):
            assert sorted(sd["output_dict_per_obj"][i][key]) == sorted(sh["output_dict_per_obj"][i][key])
            for t, e in sd["output_dict_per_obj"][i][key].items():
                f = sh["output_dict_per_obj"][i][key][t]
                for name in ("pred_masks", "obj_ptr", "maskmem_features", "object_score_logits"):
                    assert torch.equal(e[name], f[name]), (i, key, t, name)
                    n += 1
    assert n == len(IDS) * T * 4
    # and the plain results are untouched by the new keywords' defaults
    for t, seg in plain["segs"].items():
        assert sorted(seg) == ["categories", "scores"]
        assert seg["categories"] == swept["segs"][t]["categories"] and seg["scores"] == swept["segs"][t]["scores"]


def test_threshold_and_sweep_need_the_device_export():
    from sam2_video.eval import inference as I
    with pytest.raises(ValueError):
        I.predict_on_video(None, None, 0, export_on_device=False, threshold=0.4, mod=MOD)
    with pytest.raises(ValueError):
        I.predict_on_video(None, None, 0, export_on_device=True, sweep=object(), mod=MOD)
