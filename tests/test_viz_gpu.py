"""The training visualisation on the device: s2h_viz_pack / s2h_viz_compose (csrc/viz.hip through ops.viz_pack and
ops.viz_compose) against the numpy / scipy model on every case of viz_cases.py and under a captured, replayed HIP
graph; create_visualization_gif on the device against its numpy path with point, box and mask prompts; and one
short fit of this build's Trainer (Hiera-T 256^2, 4-frame clips, captured step graph) with
visualization.save_dir set against the same fit without it."""
import copy
import json
import os

import numpy as np
import pytest
import torch

import viz_cases as VC
from step_harness import GOLD
from viz_cases import clip, model_of_clip

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    cs = VC.make_cases()
    return cs, [VC.reference(c) for c in cs]


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def upload(c):
    """the case's tensors on the device; frames / masks as strided views of the stored arrays (step frames apart)"""
    s = c["step"]
    return {"frames": _dev(c["frames"])[::s], "frame0": _dev(c["frame0"]), "gt": _dev(c["gt"])[::s],
            "pred": _dev(c["pred"])[::s], "prompt": None if c["prompt"] is None else _dev(c["prompt"][None]),
            "palette": _dev(c["palette"]), "markers": _dev(c["markers"]) if len(c["markers"]) else None}


def compose(t, out=None):
    from sam2_video.kernels import ops
    pw = None if t["prompt"] is None else ops.viz_pack(t["prompt"])[0]
    return ops.viz_compose(t["frames"], t["frame0"], ops.viz_pack(t["gt"]), ops.viz_pack(t["pred"]), t["palette"],
                           t["markers"], pw, out=out)


def test_kernel_equals_model_on_every_case(cases):
    cs, refs = cases
    for c, want in zip(cs, refs):
        t = upload(c)
        if c["step"] > 1:
            assert not t["frames"].is_contiguous() and not t["gt"].is_contiguous()
        got = compose(t)
        assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape
        assert np.array_equal(got.cpu().numpy(), want), c["name"]


def test_pack_words_equal_the_threshold(cases):
    from sam2_video.kernels import ops
    cs, _ = cases
    c = next(c for c in cs if c["name"] == "130x66-n3-C64-many")
    for key in ("gt", "pred"):
        words = ops.viz_pack(_dev(c[key])).cpu().numpy().view(np.uint64)
        want = np.zeros(words.shape, np.uint64)
        for k in range(c["C"]):
            want |= (c[key][:, k] > 0.5).astype(np.uint64) << np.uint64(k)
        assert np.array_equal(words, want), key
    as_bool = ops.viz_pack(_dev(c["gt"] != 0)).cpu().numpy()
    assert np.array_equal(as_bool, ops.viz_pack(_dev(c["gt"])).cpu().numpy())


def test_kernel_under_a_replayed_graph(cases):
    from sam2_video.kernels import ops
    cs, refs = cases
    k = next(i for i, c in enumerate(cs) if c["name"] == VC.MID_CASE)
    c, t = cs[k], upload(cs[k])
    n, H, W = c["n"], c["H"], c["W"]
    gw, pw = (torch.zeros(n, H, W, dtype=torch.int64, device="cuda") for _ in range(2))
    qw = torch.zeros(1, H, W, dtype=torch.int64, device="cuda")
    out = torch.zeros(n, 2 * H, 2 * W, 3, dtype=torch.uint8, device="cuda")

    def run():
        ops.viz_pack(t["gt"], out=gw)
        ops.viz_pack(t["pred"], out=pw)
        ops.viz_pack(t["prompt"], out=qw)
        ops.viz_compose(t["frames"], t["frame0"], gw, pw, t["palette"], t["markers"], qw[0], out=out)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    for buf in (gw, pw, qw, out):
        buf.zero_()
    g.replay()
    assert np.array_equal(out.cpu().numpy(), refs[k])
    # new inputs in the same buffers: the replay reads them where they lie
    t["gt"].copy_(t["gt"].flip(-1))
    t["frame0"].copy_(t["frame0"].flip(0))
    g.replay()
    want = VC.composites(c["frames"][::c["step"]], c["frame0"][::-1], c["gt"][::c["step"], ..., ::-1],
                         c["pred"][::c["step"]], c["palette"], c["markers"], c["prompt"])
    assert np.array_equal(out.cpu().numpy(), want)


def test_limits_are_refused_without_a_launch():
    from sam2_video.kernels._lib import HipKernelError, call
    one = torch.zeros(64, dtype=torch.int64, device="cuda")
    p = one.data_ptr()
    for n, C, H, W in [(1, 1, 0, 4), (1, 1, 4, 0), (1, 0, 2, 2), (1, 65, 2, 2), (1, 1, 16384, 16384),
                       (200, 1, 1024, 1024), (-1, 1, 2, 2)]:
        with pytest.raises(HipKernelError):
            call("s2h_viz_pack", n, C, H, W, 0, p, 0, p, None)
        with pytest.raises(HipKernelError):
            call("s2h_viz_compose", n, C, H, W, 0, p, 0, p, p, p, None, p, 0, None, p, None)
    with pytest.raises(HipKernelError):
        call("s2h_viz_compose", 1, 1, 2, 2, 0, p, 0, p, p, p, None, p, 257, p, p, None)
    call("s2h_viz_compose", 0, 1, 2, 2, 0, None, 0, None, None, None, None, None, 0, None, None, None)  # n == 0


@pytest.mark.parametrize("kind", ["point", "box", "mask"])
def test_public_function_device_equals_host(kind):
    from sam2_video.utils import create_visualization_gif
    frames, gt, outs, obj_to_cat = clip(6, 13, 40, 52, 5, kind, seed=7)
    dev_outs = [{k: ([v[0].cuda()] if isinstance(v, list) else v if v is None or isinstance(v, dict) else v.cuda())
                 for k, v in o.items()} for o in outs]
    for max_length, stride in [(4, 1), (5, 2), (2, 3)]:
        host = create_visualization_gif(frames, gt, outs, obj_to_cat, max_length=max_length, stride=stride,
                                        on_device=False)
        got = create_visualization_gif(frames.cuda(), gt.cuda(), dev_outs, obj_to_cat, max_length=max_length,
                                       stride=stride)
        assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == host.shape
        assert np.array_equal(got.cpu().numpy(), host), (kind, max_length, stride)
        assert np.array_equal(host, model_of_clip(frames, gt, outs, obj_to_cat, max_length, stride))
        pinned = create_visualization_gif(frames.cuda(), gt.cuda(), dev_outs, obj_to_cat, max_length=max_length,
                                          stride=stride, to_host=True)
        assert isinstance(pinned, np.ndarray) and np.array_equal(pinned, host)
    u8 = (torch.rand(6, 40, 52, 3) * 256).to(torch.uint8)  # the viewer's image kind
    host = create_visualization_gif(u8, gt, outs, obj_to_cat, on_device=False)
    assert np.array_equal(create_visualization_gif(u8.cuda(), gt.cuda(), dev_outs, obj_to_cat).cpu().numpy(), host)


# ------------------------------------------------------------------------------------------------ the trainer hook
def _sections(save_dir):
    with open(os.path.join(GOLD, "overfit_cfg1.json")) as f:
        cfg = copy.deepcopy(json.load(f))
    for model in (cfg["model"], cfg["module"]["model"]):
        model["use_activation_checkpoint"] = False
    for data in (cfg["data"], cfg["data_module"]["data"]):
        data.update(video_clip_length=4, num_workers=0, synthetic_clips=4)
    cfg["data_module"]["train_shuffle"] = False
    cfg["module"]["visualization"].update(train_every_n_steps=2, save_dir=save_dir)
    return cfg


def _fit(save_dir, monkeypatch):
    from sam2_video.kernels import functional as FN
    from sam2_video.model.build import instantiate
    from sam2_video.training import trainer as T
    torch.manual_seed(42)
    np.random.seed(42)
    FN.set_seed(0x5EED)  # the launch seeds a fresh process starts from: both fits draw the same dropout masks
    cfg = _sections(save_dir)
    module = instantiate(cfg["module"], _recursive_=False)
    dm = instantiate(cfg["data_module"], _recursive_=False)
    steps, shots = [], []
    after = T.StepRunner.after_backward

    def recording(self, reduced=False):  # the loss and the fp32 gradient arena of every micro-step, before the step
        steps.append((self.module.logged["train/total_loss"].detach().clone(),
                      self.module.model.arena.grad.detach().clone()))
        return after(self, reduced)
    monkeypatch.setattr(T.StepRunner, "after_backward", recording)
    log = module._log_gif

    def snapshotting(stage, frames, gt_masks, outs, obj_to_cat, split):  # what the hook was handed, copied
        p0 = outs[0].get("point_inputs")
        shots.append({"stage": stage, "frames": frames.detach().cpu().clone(), "gt": gt_masks.detach().cpu().clone(),
                      "outs": [{"multistep_pred_multimasks_high_res":
                                [o["multistep_pred_multimasks_high_res"][0].detach().float().cpu().clone()],
                                "point_inputs": None, "mask_inputs": None} for o in outs],
                      "obj_to_cat": list(obj_to_cat), "capturing": torch.cuda.is_current_stream_capturing()})
        shots[-1]["outs"][0]["point_inputs"] = None if p0 is None else {k: torch.as_tensor(v).clone() for k, v in p0.items()}
        path = log(stage, frames, gt_masks, outs, obj_to_cat, split)
        shots[-1].update(path=path, array=None if path is None else module.last_visualization["array"].copy())
        return path
    module._log_gif = snapshotting
    trainer = T.Trainer(max_epochs=1, precision=16, gradient_clip_val=1.0, limit_val_batches=1, val_check_interval=1.0,
                        log_every_n_steps=1, graph=True, num_sanity_val_steps=0)
    trainer.fit(module, dm)
    torch.cuda.synchronize()
    return {"steps": steps, "shots": shots, "graphs": len(trainer.runner._graphs),
            "segs": sum(len(e["segs"]) for e in trainer.runner._graphs.values()), "history": trainer.history}


def test_fit_writes_the_scheduled_files_and_changes_nothing(tmp_path, monkeypatch):
    from PIL import Image
    save_dir = tmp_path / "viz"
    with_viz = _fit(str(save_dir), monkeypatch)
    monkeypatch.undo()
    plain = _fit(None, monkeypatch)
    # exactly the scheduled files: batches 2 and 4 (global_step 1 and 3 when they start), the epoch's validation
    assert sorted(os.listdir(save_dir)) == ["train_e0000_s0000001.gif", "train_e0000_s0000003.gif",
                                            "val_e0000_s0000004.gif"]
    shots = with_viz["shots"]
    assert [s["stage"] for s in shots] == ["train", "train", "val"] and not any(s["capturing"] for s in shots)
    assert [os.path.basename(s["path"]) for s in shots] == sorted(os.listdir(save_dir))
    assert all(s["path"] is None for s in plain["shots"]) and len(plain["shots"]) == 3  # scheduled, nothing rendered
    first = shots[0]
    assert first["frames"].shape == (4, 3, 256, 256) and first["array"].shape == (4, 3, 512, 512)
    want = model_of_clip(first["frames"], first["gt"], first["outs"], first["obj_to_cat"], 4, 1)
    assert np.array_equal(first["array"], want)
    assert first["outs"][0]["point_inputs"] is not None and len(np.unique(first["array"])) > 64
    with Image.open(first["path"]) as im:
        assert im.n_frames == 4 and im.size == (512, 512) and im.info["loop"] == 0 and im.info["duration"] == 250
        assert im.info["comment"] == b"cholecseg8k | train e0 s1"
    # the hook only reads: losses and the fp32 gradient arena of every step, bit for bit, and the same graphs
    assert len(with_viz["steps"]) == len(plain["steps"]) == 4
    for (la, ga), (lb, gb) in zip(with_viz["steps"], plain["steps"]):
        assert torch.equal(la, lb) and torch.equal(ga, gb)
    assert (with_viz["graphs"], with_viz["segs"]) == (plain["graphs"], plain["segs"]) and with_viz["graphs"] >= 1
    assert with_viz["history"] and [r["train/total_loss"] for r in with_viz["history"]] == \
        [r["train/total_loss"] for r in plain["history"]]


def test_viewer_device_equals_host(tmp_path):
    from sam2_video.eval import visualize as VIS
    want = VC.build_viewer_tree(str(tmp_path))
    args = ["--gt", str(tmp_path / "gt.json"), "--predict", str(tmp_path / "predict.json"), "--image-root", str(tmp_path),
            "--prompt", str(tmp_path / "prompt.pkl"), "--format", "png"]
    dev = VIS.main(args + ["--out", str(tmp_path / "dev")])
    host = VIS.main(args + ["--out", str(tmp_path / "host"), "--host"])
    assert [os.path.basename(f) for f in dev] == [os.path.basename(f) for f in host] and len(dev) == 6
    for name, parts in want.items():
        got = VC.read_png_series(tmp_path / "dev", name)
        assert np.array_equal(got, VC.read_png_series(tmp_path / "host", name)), name
        assert np.array_equal(got, VC.viewer_model(parts)), name
