"""Prompts from ground truth on the device (csrc/gtprompt.hip): the RLE decoder, the rectangular morphology, the
component listing and the rank selection against the numpy / scipy models of gt_prompt_ref.py, exactly; then
eval/inference.py get_each_obj on both paths against the test's own model, and inference() + eval() end to end
on the small predictor of test_inference_export_gpu.py."""
import json
import os
import pickle

import numpy as np
import pytest
import torch

import cc_patterns as cp
import gt_prompt_ref as R
from sam2_video.data import rle

pytestmark = pytest.mark.gpu


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


# ------------------------------------------------------------------------------------------------ decode
@pytest.mark.parametrize("shape", R.DECODE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_rle_decode_patterns(shape):
    from sam2_video.kernels import ops
    H, W = shape
    pats = R.decode_patterns(H, W)
    counts = [R.counts_of(m) for m in pats.values()]
    if H * W > 1:
        assert counts[list(pats).index("first")][0] == 0 and len(counts[list(pats).index("empty")]) == 1
    got = ops.rle_decode(counts, H, W).cpu().numpy()  # six annotations with different run counts in one call
    assert got.dtype == np.uint8 and got.shape == (len(pats), H, W)
    for k, (name, c) in enumerate(zip(pats, counts)):
        assert np.array_equal(got[k], rle.decode({"size": [H, W], "counts": c})), name
        assert np.array_equal(got[k], pats[name].astype(np.uint8)), name
        assert np.array_equal(ops.rle_decode([c], H, W).cpu().numpy()[0], got[k]), name
    assert ops.rle_decode([], H, W).shape == (0, H, W)


def test_rle_decode_golden_annotations():
    from sam2_video.kernels import ops
    anns = R.golden_annotations()
    assert len(anns) == 48 and len({(h, w) for h, w, _, _ in anns}) == 1
    H, W = anns[0][:2]
    got = ops.rle_decode([c for _, _, c, _ in anns], H, W).cpu().numpy()
    for k, (_, _, _, want) in enumerate(anns):
        assert np.array_equal(got[k], want), k


def test_rle_decode_rejects_bad_counts():
    from sam2_video.kernels import ops
    for bad in ([[5, 5]], [[10, -1, 3]], [[]]):
        with pytest.raises(ValueError):
            ops.rle_decode(bad, 3, 4)


# ------------------------------------------------------------------------------------------------ morphology
@pytest.mark.parametrize("shape", R.MORPH_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_morph_rect(shape):
    from sam2_video.kernels import ops
    H, W = shape
    pats = R.morph_patterns(H, W)
    names = list(pats)
    single = _dev(np.stack([pats[k] for k in names]), torch.uint8)  # N = 5 ...
    triple = _dev(np.stack([pats[k] for k in names[2:5]]).astype(np.uint8) * 255)  # ... N = 3 with bytes of 255
    for yw, xw in R.WINDOWS:
        for op in (0, 1):
            want = np.stack([R.morph_model(pats[k], op, yw, xw) for k in names]).astype(np.uint8)
            got = ops.morph_rect(single, op, yw, xw).cpu().numpy()
            assert np.array_equal(got, want), (yw, xw, op)
            assert np.array_equal(ops.morph_rect(triple, ("dilate", "erode")[op], yw, xw).cpu().numpy(), want[2:5])
            for k in (0, 2, 4):  # N = 1
                assert np.array_equal(ops.morph_rect(single[k:k + 1], op, yw, xw).cpu().numpy()[0], want[k]), names[k]


def test_morph_rect_rejects_bad_arguments():
    from sam2_video.kernels import _lib, ops
    m = torch.zeros(1, 4, 4, dtype=torch.uint8, device="cuda")
    for yw, xw in (((-33, 0), (0, 0)), ((0, 33), (0, 0)), ((1, 2), (0, 0)), ((0, 0), (-2, -1))):
        with pytest.raises(ValueError):
            ops.morph_rect(m, 0, yw, xw)
    out, work = torch.empty_like(m), torch.empty_like(m)
    with pytest.raises(_lib.HipKernelError):  # out aliases in
        _lib.call("s2h_morph_rect", 1, 4, 4, m.data_ptr(), 0, -1, 1, -1, 1, m.data_ptr(), work.data_ptr(), None)
    with pytest.raises(_lib.HipKernelError):  # op
        _lib.call("s2h_morph_rect", 1, 4, 4, m.data_ptr(), 2, -1, 1, -1, 1, out.data_ptr(), work.data_ptr(), None)
    with pytest.raises(_lib.HipKernelError):  # sizes beyond 2^24 pixels per image
        _lib.call("s2h_morph_rect", 1, 4097, 4096, m.data_ptr(), 0, -1, 1, -1, 1, out.data_ptr(), work.data_ptr(), None)


# ------------------------------------------------------------------------------------------------ components
def test_byte_labelling_is_the_float_labelling():
    from sam2_video.kernels import ops
    names, scores, ref = cp.shape_case(65, 130)
    s = _dev(scores)
    for positive in (True, False):
        m = ((s > 0) if positive else (s <= 0)).to(torch.uint8) * 7
        lab, area = ops.cc_label_u8(m, positive=True)
        lf, af = ops.cc_label(s, positive=positive)
        assert torch.equal(lab, lf) and torch.equal(area, af)
        assert np.array_equal(lab.cpu().numpy(), ref[positive][0]) and np.array_equal(area.cpu().numpy(), ref[positive][1])
    lab0, _ = ops.cc_label_u8((s > 0).to(torch.uint8), positive=False)
    assert np.array_equal(lab0.cpu().numpy(), ref[False][0])  # the zero bytes as foreground


@pytest.mark.parametrize("case", R.component_cases(), ids=lambda c: c[0])
def test_cc_components(case):
    from sam2_video.kernels import _lib, ops
    name, binary, min_area, grid, capacity = case
    N, H, W = binary.shape
    labels, areas = ops.cc_label_u8(_dev(binary, torch.uint8))
    grid_d = None if grid is None else _dev(grid, torch.uint8)
    # own buffers: one row more than the capacity, prefilled, shows that nothing is written past the end
    hdr = torch.full((2 * N + 2,), -7, dtype=torch.int32, device="cuda")
    stats = torch.full((capacity + 1, 9), -7, dtype=torch.int64, device="cuda")
    index = torch.full((N, H, W), 99, dtype=torch.uint8, device="cuda")
    work = torch.empty(N * H * W + N * ((H * W + 255) // 256), dtype=torch.int32, device="cuda")
    _lib.call("s2h_cc_components", N, H, W, labels.data_ptr(), areas.data_ptr(), min_area,
              None if grid_d is None else grid_d.data_ptr(), capacity, hdr.data_ptr(), stats.data_ptr(),
              index.data_ptr(), work.data_ptr(), torch.cuda.current_stream().cuda_stream)
    stats_h = stats.cpu().numpy()
    counts = R.check_components(name, binary, min_area, grid, capacity, hdr.cpu().numpy(), stats_h, index.cpu().numpy())
    assert np.all(stats_h[min(sum(counts), capacity):] == -7), name
    # the wrapper (default capacity 255 N) returns the same
    h2, s2, i2 = ops.cc_components(labels, areas, min_area, grid=grid_d)
    n = min(sum(counts), 255 * N)
    assert torch.equal(h2, hdr) and torch.equal(i2, index) and s2.shape == (255 * N, 9)
    assert np.array_equal(s2[:n].cpu().numpy()[:min(n, capacity)], stats_h[:min(n, capacity)])


# ------------------------------------------------------------------------------------------------ rank select
@pytest.mark.parametrize("case", R.rank_cases(), ids=lambda c: c[0])
def test_mask_rank_select(case):
    from sam2_video.kernels import ops
    name, labels, grid, qs = case
    q = _dev(np.asarray(qs, np.int32).T)
    xy, count = ops.mask_rank_select(q[0].contiguous(), q[1].contiguous(), q[2].contiguous(), q[3].contiguous(),
                                     _dev(labels.astype(np.int32)), grid=None if grid is None else _dev(grid, torch.uint8))
    R.check_ranks(name, labels, grid, qs, xy.cpu().numpy(), count.cpu().numpy())


# ------------------------------------------------------------------------------------------------ get_each_obj
@pytest.fixture
def grid_state():
    from sam2_video.eval import utils as U
    saved = U.GRID
    yield U
    U.GRID = saved


def _same_objs(objs, want):
    assert len(objs) == len(want)
    for o, (obj_id, bbox, points, labels, mask) in zip(objs, want):
        assert o.obj_id == obj_id and o.bbox == bbox and all(isinstance(v, float) for v in o.bbox)
        assert o.points.dtype == points.dtype and np.array_equal(o.points, points)
        assert o.pos_or_neg_label.dtype == labels.dtype and np.array_equal(o.pos_or_neg_label, labels)
        assert o.mask.dtype == bool and np.array_equal(o.mask, mask)


@pytest.mark.parametrize("spacing", [None, 4])
@pytest.mark.parametrize("num_neg_points", [0, 2])
@pytest.mark.parametrize("include_center", [True, False])
@pytest.mark.parametrize("num_points", [1, 3])
def test_get_each_obj_device_host_and_model_agree(grid_state, num_points, include_center, num_neg_points, spacing):
    from sam2_video.eval import inference as I
    U = grid_state
    coco_dict, frame = R.prompt_frame_case()
    coco = I.CocoIndex(coco_dict)
    assert coco.mod == 3
    U.GRID = None
    if spacing is not None:
        U.init_grid((48, 80), spacing)
    kw = dict(mod=coco.mod, obj_count=5, num_points=num_points, num_neg_points=num_neg_points,
              include_center=include_center)
    results, states = [], []
    for on_device in (True, False):
        np.random.seed(123)
        objs, count = I.get_each_obj(coco, frame, on_device=on_device, **kw)
        states.append(np.random.get_state()[1].copy())
        results.append((objs, count))
    np.random.seed(123)
    want, want_count = R.objs_model(coco_dict["annotations"], coco.mod, 5, num_points, num_neg_points, include_center,
                                    R.make_grid(48, 80, spacing))
    states.append(np.random.get_state()[1].copy())
    # annotation 1 closes into two components (the speck is dropped), 2 and 3 into one each
    assert [w[0] for w in want] == [5 * 3 + 1, 6 * 3 + 1, 7 * 3 + 2, 8 * 3 + 1] and want_count == 9
    for objs, count in results:
        assert count == want_count
        _same_objs(objs, want)
    assert np.array_equal(states[0], states[1]) and np.array_equal(states[0], states[2])
    k = num_points + num_neg_points
    assert all(len(o.points) == k for o in results[0][0])
    # a category filter keeps the object numbering of what is left
    np.random.seed(123)
    only2, c2 = I.get_each_obj(coco, frame, cats={2}, on_device=True, **kw)
    assert c2 == 6 and [o.obj_id for o in only2] == [5 * 3 + 2] and np.array_equal(only2[0].mask, want[2][4])


def test_get_each_obj_quirks_on_both_paths(grid_state):
    """more points asked than there are: all of them, no centre; zero points with the centre raises"""
    from sam2_video.eval import inference as I
    U = grid_state
    coco_dict, frame = R.prompt_frame_case()
    coco = I.CocoIndex(coco_dict)
    U.GRID = None
    U.init_grid((48, 80), 8)
    got = []
    for on_device in (True, False):
        np.random.seed(1)
        got.append(I.get_each_obj(coco, frame, mod=3, obj_count=0, num_points=50, num_neg_points=0,
                                  include_center=True, on_device=on_device)[0])
    np.random.seed(1)
    want, _ = R.objs_model(coco_dict["annotations"], 3, 0, 50, 0, True, R.make_grid(48, 80, 8))
    for objs in got:
        _same_objs(objs, want)
    assert all(len(o.points) == int((o.mask & U.GRID).sum()) < 49 for o in got[0])
    for on_device in (True, False):
        with pytest.raises(ValueError):
            I.get_each_obj(coco, frame, mod=3, obj_count=0, num_points=0, num_neg_points=0, include_center=True,
                           on_device=on_device)
    assert I.get_each_obj(coco, {"id": 12345}, mod=3, obj_count=4, num_points=1, num_neg_points=0,
                          include_center=True) == ([], 4)


# ------------------------------------------------------------------------------------------------ inference()
S, FH, FW = 256, 64, 96


@pytest.fixture(scope="module")
def predictor():
    from step_harness import build_model
    from sam2_video.predictor import SAM2VideoPredictor
    return SAM2VideoPredictor(build_model("tiny", S, [], "point", dtype="bf16", seed=3), fill_hole_area=8)


@pytest.fixture(scope="module")
def coco_file(tmp_path_factory):
    """2 videos of 3 JPEG frames of 64 x 96, categories 1 and 2; frame 0 of the second video is no keyframe"""
    from PIL import Image
    root = tmp_path_factory.mktemp("gt_coco")
    rng = np.random.default_rng(0)
    images, anns = [], []
    for v, video in enumerate(("a", "b")):
        for t in range(3):
            path = root / f"{video}_{t}.jpg"
            Image.fromarray(rng.integers(0, 256, (FH, FW, 3), dtype=np.uint8)).save(path, quality=95)
            image_id = 10 * v + t + 1
            images.append({"id": image_id, "video_id": video, "order_in_video": t, "height": FH, "width": FW,
                           "path": str(path), "file_name": path.name, "is_det_keyframe": not (v == 1 and t == 0)})
            for cat, (y, x) in ((1, (8 + 3 * t, 10 + 5 * v)), (2, (34, 50 + 4 * t))):
                m = np.zeros((FH, FW), bool)
                m[y:y + 18, x:x + 26] = True
                m[y + 6:y + 9, x + 8:x + 12] = False
                anns.append({"id": len(anns) + 1, "image_id": image_id, "category_id": cat,
                             "segmentation": rle.encode(m), "iscrowd": 0, "area": int(m.sum())})
    coco = {"images": images, "annotations": anns, "categories": [{"id": 1, "name": "one"}, {"id": 2, "name": "two"}]}
    path = root / "coco.json"
    path.write_text(json.dumps(coco))
    return str(path), coco


def _same_prompt_infos(a, b):
    assert len(a) == len(b) > 0
    for p, q in zip(a, b):
        assert (p.frame_idx, p.prompt_type, p.video_id, p.path, p.clip_range) == \
               (q.frame_idx, q.prompt_type, q.video_id, q.path, q.clip_range)
        _same_objs(p.prompt_objs, [(o.obj_id, o.bbox, o.points, o.pos_or_neg_label, o.mask) for o in q.prompt_objs])


@pytest.mark.parametrize("prompt_type", ["points", "bbox", "mask"])
def test_inference_end_to_end(predictor, coco_file, tmp_path, prompt_type):
    from sam2_video.eval import eval as E
    from sam2_video.eval import inference as I
    from sam2_video.eval import utils as U
    coco_path, coco = coco_file
    assert U.GRID is None
    texts, prompts = [], []
    for k, on_device in enumerate((True, False)):
        np.random.seed(5)
        predict_path, prompt_path = I.inference(coco_path, None, prompt_type, num_points=2, num_neg_points=1,
                                                run_dir=str(tmp_path / f"run{k}"), predictor=predictor,
                                                prompts_on_device=on_device)
        assert predict_path == str(tmp_path / f"run{k}" / "eval" / "predict.json")
        assert prompt_path == str(tmp_path / f"run{k}" / "eval" / "prompt.pkl")
        texts.append(open(predict_path, "rb").read())
        with open(prompt_path, "rb") as f:
            prompts.append(pickle.load(f))
    assert texts[0] == texts[1] and len(json.loads(texts[0])) > 0
    _same_prompt_infos(prompts[0], prompts[1])
    # the same clips by hand: host-generated PromptInfo lists into process_video_clip + save_as_coco_format
    index = I.CocoIndex(coco_path)
    gen = I.PromptGen(index, num_points=2, num_neg_points=1, include_center=True, on_device=False)
    np.random.seed(5)
    segments, log = {}, []
    for video_id in ("a", "b"):
        frames = index.frames(video_id)
        gen.obj_count = 0
        clips = list(I.generate_prompts_by_clip_length(gen, frames, prompt_type, None))
        assert [(c.start_idx, c.end_idx) for _, c in clips] == [(0, 2)]
        assert [p.frame_idx for p in clips[0][0]] == [0 if video_id == "a" else 1]  # b's frame 0 is no keyframe
        log += clips[0][0]
        segments[video_id] = I.process_video_clip(predictor, frames, clips[0][0], clips[0][1], mod=index.mod)
    by_hand, _ = I.save_as_coco_format(segments, {v: index.frames(v) for v in ("a", "b")}, index.mod,
                                       str(tmp_path / "by_hand"), prompt_info=log)
    assert open(by_hand, "rb").read() == texts[0]
    _same_prompt_infos(prompts[0], log)
    assert [o.obj_id for o in log[0].prompt_objs] == [1, 3 + 2] and log[0].prompt_type == prompt_type
    # eval() on the result
    out = tmp_path / "run0"
    res = E.eval(str(out / "eval" / "predict.json"), coco_path, str(out))
    with open(out / "eval.pkl", "rb") as f:
        stored = pickle.load(f)
    want = R.eval_model(coco, json.loads(texts[0]), [1, 2])
    for key in E.KEYS:
        assert np.isfinite(res["avg_scores"][key]) and res["avg_scores"][key] == stored["avg_scores"][key] == want[key]
    assert [v["video_id"] for v in res["videos"]] == ["a", "b"] and [len(v["frames"]) for v in res["videos"]] == [3, 2]


def test_inference_writes_the_dump_meta(predictor, coco_file, tmp_path):
    from sam2_video.eval import inference as I
    coco_path, _ = coco_file
    np.random.seed(0)
    I.inference(coco_path, None, "point", run_dir=str(tmp_path), predictor=predictor, probs_out_dir="probs",
                save_video_list=["b"])
    probs = tmp_path / "eval" / "probs"
    meta = json.loads((probs / "meta.json").read_text())
    assert meta["mod"] == 3 and meta["dtype"] == "float16" and meta["image_ids"] == [1, 2, 3, 11, 12, 13]
    anns = json.loads((tmp_path / "eval" / "predict.json").read_text())
    assert {a["image_id"] for a in anns} <= {11, 12, 13} and anns  # save_video_list: only video b is written
    with open(tmp_path / "eval" / "prompt.pkl", "rb") as f:
        assert [p.video_id for p in pickle.load(f)] == ["a", "b"]  # this call's prompts only
