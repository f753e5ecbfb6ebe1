"""Correction clicks on the device (csrc/clicks.hip): the squared distance transform, the centre click and the
uniform click against the numpy models of click_cases.py, exactly, on every pattern and shape of the host test;
model/modeling/sam2_utils.py on the device against its host twin; one case at 1024 x 1280 from real annotations;
and inference() with corrective clicks end to end on the small predictor of test_gt_prompts_gpu.py, device
against host clicks."""
import json
import pickle

import numpy as np
import pytest
import torch

import click_cases as C
from sam2_video.data import rle

pytestmark = pytest.mark.gpu

IDS = [f"{h}x{w}" for h, w in C.SHAPES]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _u8(masks):
    return _dev(np.stack(masks).astype(np.uint8))


def _batches(H, W):
    """the pairs of a shape as two batches [(name, gt, pred)]: those with a prediction and those without"""
    pairs = C.pair_patterns(H, W)
    return ([(n, g, p) for n, (g, p) in pairs.items() if p is not None],
            [(n, g, None) for n, (g, p) in pairs.items() if p is None])


# ------------------------------------------------------------------------------------------------ the transform
@pytest.mark.parametrize("shape", C.SHAPES, ids=IDS)
def test_edt_sq(shape):
    from sam2_video.kernels import ops
    H, W = shape
    pats = C.mask_patterns(H, W)
    want = {name: C.d2_model(m) for name, m in pats.items()}
    for name, m in pats.items():
        got = ops.edt_sq(_u8([m]) * 255)
        assert got.dtype == torch.int32 and got.shape == (1, H, W)
        assert np.array_equal(got.cpu().numpy()[0], want[name]), name
    names = list(pats)[3:8]  # five different patterns side by side
    got = ops.edt_sq(_u8([pats[n] for n in names])).cpu().numpy()
    for k, n in enumerate(names):
        assert np.array_equal(got[k], want[n]), n
    assert ops.edt_sq(torch.zeros(0, H, W, dtype=torch.uint8, device="cuda")).shape == (0, H, W)


def test_entries_reject_bad_sizes():
    from sam2_video.kernels import _lib, ops
    with pytest.raises(ValueError):
        ops.edt_sq(torch.zeros(1, 2, 4093, dtype=torch.uint8, device="cuda"))
    m = torch.zeros(1, 4, 4, dtype=torch.uint8, device="cuda")
    out = torch.zeros(64, dtype=torch.int64, device="cuda")
    for name, args in (("s2h_edt_sq", (1, 4093, 4, m.data_ptr(), out.data_ptr(), out.data_ptr(), None)),
                       ("s2h_edt_sq", (1, 4, 4, None, out.data_ptr(), out.data_ptr(), None)),
                       ("s2h_error_center_click", (1, 4, 0, m.data_ptr(), None, out.data_ptr(), out.data_ptr(),
                                                   out.data_ptr(), out.data_ptr(), None)),
                       ("s2h_error_uniform_click", (1, -1, 4, 4, m.data_ptr(), None, out.data_ptr(), out.data_ptr(),
                                                    out.data_ptr(), out.data_ptr(), out.data_ptr(), None))):
        with pytest.raises(_lib.HipKernelError):
            _lib.call(name, *args)


# ------------------------------------------------------------------------------------------------ the clicks
@pytest.mark.parametrize("shape", C.SHAPES, ids=IDS)
def test_error_center_click(shape):
    from sam2_video.kernels import ops
    H, W = shape
    for batch in _batches(H, W):
        want = [C.center_model(g, p) for _, g, p in batch]
        gt = _u8([g for _, g, _ in batch])
        pred = None if batch[0][2] is None else _u8([p for _, _, p in batch]) * 7
        points, labels, dmax = ops.error_center_click(gt, pred)
        assert points.dtype == torch.float32 and labels.dtype == torch.int32 and dmax.dtype == torch.int32
        points, labels, dmax = points.cpu().numpy(), labels.cpu().numpy(), dmax.cpu().numpy()
        for b, (xy, label, d) in enumerate(want):
            assert (tuple(points[b]), labels[b], tuple(dmax[b])) == (xy, label, d), batch[b][0]
        for b in range(0, len(batch), 3):  # and alone
            one = ops.error_center_click(gt[b:b + 1], None if pred is None else pred[b:b + 1])
            assert (tuple(one[0][0].tolist()), int(one[1][0]), tuple(one[2][0].tolist())) == want[b], batch[b][0]


@pytest.mark.parametrize("shape", C.SHAPES, ids=IDS)
def test_error_uniform_click(shape):
    from sam2_video.kernels import ops
    H, W = shape
    for batch in _batches(H, W):
        draws = [C.draws_for(g, p) for _, g, p in batch]
        P = max(len(d) for d in draws)
        r = np.asarray([d + [0] * (P - len(d)) for d in draws], np.int64)
        want = [C.uniform_model(g, p, r[b]) for b, (_, g, p) in enumerate(batch)]
        gt = _u8([g for _, g, _ in batch])
        pred = None if batch[0][2] is None else _u8([p for _, _, p in batch])
        points, labels, count = ops.error_uniform_click(gt, pred, _dev(r))
        assert points.shape == (len(batch), P, 2) and points.dtype == torch.float32 and labels.dtype == torch.int32
        points, labels, count = points.cpu().numpy(), labels.cpu().numpy(), count.cpu().numpy()
        for b, (pts, lab, cnt) in enumerate(want):
            assert np.array_equal(points[b], pts) and np.array_equal(labels[b], lab), batch[b][0]
            assert tuple(count[b]) == cnt, batch[b][0]
        none = ops.error_uniform_click(gt, pred, torch.zeros(len(batch), 0, dtype=torch.int64, device="cuda"))
        assert none[0].shape == (len(batch), 0, 2) and np.array_equal(none[2].cpu().numpy(), count)


@pytest.mark.parametrize("shape", [(5, 64), (65, 130)], ids=["5x64", "65x130"])
def test_sam2_utils_device_equals_host_twin(shape):
    from sam2_video.model.modeling import sam2_utils as U
    H, W = shape
    for batch in _batches(H, W):
        gt = _dev(np.stack([g for _, g, _ in batch]))[:, None]
        pred = None if batch[0][2] is None else _dev(np.stack([p for _, _, p in batch]))[:, None]
        B = len(batch)
        dev = U.sample_one_point_from_error_center(gt, pred)
        host = U.sample_one_point_from_error_center(gt, pred, on_device=False)
        assert dev[0].shape == (B, 1, 2) and dev[0].dtype == torch.float32 and dev[0].is_cuda and host[0].is_cuda
        assert dev[1].shape == (B, 1) and dev[1].dtype == torch.int32
        assert torch.equal(dev[0], host[0]) and torch.equal(dev[1], host[1])
        for b, (_, g, p) in enumerate(batch):
            xy, label, _ = C.center_model(g, p)
            assert tuple(dev[0][b, 0].tolist()) == xy and int(dev[1][b, 0]) == label
        for num_pt in (1, 4):
            both = [U.sample_random_points_from_errors(gt, pred, num_pt=num_pt, on_device=on_device,
                                                       generator=torch.Generator(device="cuda").manual_seed(5))
                    for on_device in (True, False)]
            assert both[0][0].shape == (B, num_pt, 2) and both[0][1].shape == (B, num_pt)
            assert both[0][0].dtype == torch.float32 and both[0][1].dtype == torch.int32
            assert torch.equal(both[0][0], both[1][0]) and torch.equal(both[0][1], both[1][1])
            r = torch.randint(0, 2 ** 32, (B, num_pt), dtype=torch.int64, device="cuda",
                              generator=torch.Generator(device="cuda").manual_seed(5)).cpu().numpy()
            for b, (_, g, p) in enumerate(batch):
                pts, lab, _ = C.uniform_model(g, p, r[b])
                assert np.array_equal(both[0][0][b].cpu().numpy(), pts)
                assert np.array_equal(both[0][1][b].cpu().numpy(), lab)
        for method in ("center", "uniform"):
            gens = [torch.Generator(device="cuda").manual_seed(9) for _ in range(2)]
            a = U.get_next_point(gt, pred, method, generator=gens[0])
            b = U.get_next_point(gt, pred, method, generator=gens[1], on_device=False)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[0].shape == (B, 1, 2)


def test_real_annotations_at_full_resolution():
    """two annotations of the EndoVis sample (1024 x 1280) against themselves shifted and eroded"""
    import gt_prompt_ref as R
    from sam2_video.kernels import ops
    anns = sorted(R.golden_annotations(), key=lambda a: -int(a[3].sum()))[:2]
    H, W = anns[0][:2]
    assert (H, W) == (1024, 1280)
    gt = np.stack([a[3] for a in anns]).astype(bool)
    gt_d = _u8(list(gt))
    shifted = _u8([np.roll(gt[0], (3, -5), (0, 1)), np.roll(gt[1], (-2, 4), (0, 1))])
    pred_d = ops.morph_rect(shifted, "erode", (-2, 2), (-1, 1))
    pred = pred_d.cpu().numpy().astype(bool)
    assert all((gt[b] & ~pred[b]).sum() > 100 and (~gt[b] & pred[b]).sum() > 100 for b in range(2))
    points, labels, dmax = ops.error_center_click(gt_d, pred_d)
    again = ops.error_center_click(gt_d, pred_d)
    r = torch.randint(0, 2 ** 32, (2, 6), dtype=torch.int64, device="cuda",
                      generator=torch.Generator(device="cuda").manual_seed(1))
    u = ops.error_uniform_click(gt_d, pred_d, r)
    u_again = ops.error_uniform_click(gt_d, pred_d, r)
    for a, b in zip((points, labels, dmax) + u, again + u_again):  # two calls: identical bytes
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    fn_d2 = ops.edt_sq(gt_d * (1 - pred_d))  # (bytes 0 / 1: gt & ~pred)
    for b in range(2):
        xy, label, d = C.center_model(gt[b], pred[b], d2=C.d2_separable)
        assert (tuple(points[b].tolist()), int(labels[b]), tuple(dmax[b].tolist())) == (xy, label, d)
        assert d[0] > 1 and d[1] > 1
        pts, lab, cnt = C.uniform_model(gt[b], pred[b], r[b].cpu().numpy())
        assert np.array_equal(u[0][b].cpu().numpy(), pts) and np.array_equal(u[1][b].cpu().numpy(), lab)
        assert tuple(u[2][b].tolist()) == cnt
        assert np.array_equal(fn_d2[b].cpu().numpy(), C.d2_separable(gt[b] & ~pred[b]))


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
    root = tmp_path_factory.mktemp("click_coco")
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
    return str(path)


def _run(predictor, coco_path, run_dir, prompt_type, **kw):
    from sam2_video.eval import inference as I
    np.random.seed(5)
    predict_path, prompt_path = I.inference(coco_path, None, prompt_type, num_points=2, num_neg_points=1,
                                            run_dir=str(run_dir), predictor=predictor, **kw)
    with open(prompt_path, "rb") as f:
        return open(predict_path, "rb").read(), pickle.load(f)


def _same_prompts(a, b):
    assert len(a) == len(b) > 0
    for p, q in zip(a, b):
        assert (p.frame_idx, p.prompt_type, p.video_id, p.path, p.clip_range) == \
               (q.frame_idx, q.prompt_type, q.video_id, q.path, q.clip_range)
        assert len(p.prompt_objs) == len(q.prompt_objs) > 0
        for o, w in zip(p.prompt_objs, q.prompt_objs):
            assert o.obj_id == w.obj_id and o.bbox == w.bbox and np.array_equal(o.mask, w.mask)
            assert o.points.dtype == w.points.dtype and np.array_equal(o.points, w.points)
            assert o.pos_or_neg_label.dtype == w.pos_or_neg_label.dtype
            assert np.array_equal(o.pos_or_neg_label, w.pos_or_neg_label)


@pytest.mark.parametrize("prompt_type", ["point", "bbox"])
def test_inference_with_correction_clicks(predictor, coco_file, tmp_path, prompt_type):
    base_text, base_prompts = _run(predictor, coco_file, tmp_path / "base", prompt_type)
    zero_text, zero_prompts = _run(predictor, coco_file, tmp_path / "zero", prompt_type, num_correction_clicks=0)
    assert zero_text == base_text and len(json.loads(base_text)) > 0  # no clicks: the bytes of a call without them
    _same_prompts(zero_prompts, base_prompts)
    dev_text, dev_prompts = _run(predictor, coco_file, tmp_path / "dev", prompt_type, num_correction_clicks=2,
                                 clicks_on_device=True)
    host_text, host_prompts = _run(predictor, coco_file, tmp_path / "host", prompt_type, num_correction_clicks=2,
                                   clicks_on_device=False)
    assert dev_text == host_text and len(json.loads(dev_text)) > 0
    _same_prompts(dev_prompts, host_prompts)
    for p, q in zip(dev_prompts, base_prompts):
        for o, w in zip(p.prompt_objs, q.prompt_objs):  # every object's logged points grow by exactly two
            assert len(o.points) == len(w.points) + 2 == len(o.pos_or_neg_label)
            assert np.array_equal(o.points[:-2], w.points) and np.array_equal(o.pos_or_neg_label[:-2], w.pos_or_neg_label)
            assert set(o.pos_or_neg_label[-2:].tolist()) <= {0.0, 1.0}
            assert (o.points[-2:] >= 0).all() and (o.points[-2:, 0] < FW).all() and (o.points[-2:, 1] < FH).all()


def test_inference_with_uniform_clicks(predictor, coco_file, tmp_path):
    kw = dict(num_correction_clicks=1, correction_method="uniform")
    dev_text, dev_prompts = _run(predictor, coco_file, tmp_path / "dev", "point", clicks_on_device=True, **kw)
    host_text, host_prompts = _run(predictor, coco_file, tmp_path / "host", "point", clicks_on_device=False, **kw)
    assert dev_text == host_text and len(json.loads(dev_text)) > 0
    _same_prompts(dev_prompts, host_prompts)
    assert all(len(o.points) == 3 + 1 for p in dev_prompts for o in p.prompt_objs)
