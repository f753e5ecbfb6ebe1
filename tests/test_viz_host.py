"""The training visualisation without a GPU: the blend identity, csrc/viz_pixel.h compiled for the host and run
pixel after pixel (csrc/viz_host_check.cpp: a stand-alone program, built plain and under the address and
undefined-behaviour sanitizers) against the numpy / scipy model of viz_cases.py on every case, the package's numpy
path (create_visualization_gif(on_device=False)) with the reference's frame selection, the schedule
(_should_log_gif) and the Pillow writer."""
import json
import os
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import viz_cases as VC
from viz_cases import clip, model_of_clip
from sam2_video.training.trainer import SAM2LightningModule
from sam2_video.utils import create_visualization_gif, save_visualization
from sam2_video.utils import viz as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sam2-video-training_amd", "csrc")


def test_blend_identity_over_all_pairs():
    """(4 b + o + 2) / 5 in integers == rint(0.8 b + 0.2 o) in float64 == cv2.addWeighted's saturate_cast: the
    fraction is a multiple of 0.2, never a tie"""
    b, o = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    want = np.rint(b.astype(np.float64) * 0.8 + o.astype(np.float64) * 0.2)
    assert np.array_equal((4 * b + o + 2) // 5, want.astype(np.int64))
    assert np.abs((b * 0.8 + o * 0.2) % 1 - 0.5).min() > 0.05  # no value near a tie
    assert np.array_equal(VC.blend(b.astype(np.uint8), o.astype(np.uint8)), want.astype(np.uint8))


@pytest.fixture(scope="module")
def cases():
    cs = VC.make_cases()
    return cs, [VC.reference(c) for c in cs]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def host_check(request, tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build csrc/viz_host_check.cpp")
    exe = tmp_path_factory.mktemp("viz_host") / f"viz_host_check_{request.param}"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", *flags, "-I", CSRC,
                    os.path.join(CSRC, "viz_host_check.cpp"), "-o", str(exe)], check=True)
    return str(exe)


def test_the_cases_cover_what_they_claim(cases):
    cs, refs = cases
    by_name = {c["name"]: c for c in cs}
    assert {(c["H"], c["W"]) for c in cs} == set(VC.SIZES)
    assert any(W % 2 for _, W in VC.SIZES) and any(H * W % 4 for H, W in VC.SIZES)  # rows / frames off the dwords
    for H, W in VC.SIZES:
        here = [c for c in cs if (c["H"], c["W"]) == (H, W)]
        assert {c["n"] for c in here} == {1, 3} and {c["C"] for c in here} >= {1, 13, 64}
        assert {c["frames"].dtype for c in here} == {np.dtype(np.uint8), np.dtype(np.float32)}
        assert {(c["gt"].dtype, c["pred"].dtype) for c in here} >= {(np.dtype(np.uint8), np.dtype(np.float32)),
                                                                    (np.dtype(np.float32), np.dtype(np.uint8))}
        assert any(c["step"] == 2 and c["n"] == 3 for c in here) and any(c["prompt"] is not None for c in here)
    assert {len(c["markers"]) for c in cs} >= {0, 5, 8, 256}
    c = by_name["17x33-n3-C64-levels"]
    for ch in range(3):  # every level of every channel, and both values beyond the range
        want = ((np.arange(256) / 255.0 - VC.MEAN[ch]) / VC.STD[ch]).astype(np.float32)
        assert set(want.tolist()) | {-5.0, 5.0} <= set(c["frames"][0, ch].ravel().tolist())
    u8 = VC.frame_u8(c["frames"])
    assert u8.min() == 0 and u8.max() == 255 and len(np.unique(u8)) >= 240  # (truncation maps some p to p - 1)
    logits = by_name["130x66-n3-C64-many"]["pred"]
    for v in VC.SPECIAL_LOGITS:
        assert ((logits == v) & (np.signbit(logits) == np.signbit(v))).any(), v
    assert np.float32(0.5) < VC.SPECIAL_LOGITS[1] and not (np.float32(0.5) > 0.5)
    pats = VC.patterns(17, 33)
    assert not pats["empty"].any() and pats["full"].all() and (~pats["hole"]).sum() == 1
    assert pats["corner_tl"][0, 0] and pats["corner_br"][-1, -1] and pats["left"][:, 0].all() and pats["top"][0].any()
    # the band: a hole is outlined, the image border is not
    pal = VC.palette_of(1)
    base = np.zeros((17, 33, 3), np.uint8)
    ring = VC.overlay_panel(base, pats["hole"][None].astype(np.uint8), pal)
    assert (ring[7:10, 15:18] == pal[0]).all() and not (ring[0, 0] == pal[0]).all()


def run_host(exe, cases, tmp_path):
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        for c in cases:
            f.write(VC.case_bytes(c))
    subprocess.run([exe, str(src), str(dst)], check=True, timeout=300)
    raw, out, off = dst.read_bytes(), [], 0
    for c in cases:
        shape = (c["n"], 2 * c["H"], 2 * c["W"], 3)
        out.append(np.frombuffer(raw, np.uint8, int(np.prod(shape)), off).reshape(shape))
        off += int(np.prod(shape))
    assert off == len(raw)
    return out


def test_host_model_equals_numpy(host_check, cases, tmp_path):
    cs, refs = cases
    for c, got, want in zip(cs, run_host(host_check, cs, tmp_path), refs):
        assert np.array_equal(got, want), c["name"]


def test_host_check_refuses_sizes_beyond_the_limits(host_check, tmp_path):
    dst = tmp_path / "out.bin"
    for k, hdr in enumerate([(1, 1, 0, 4), (1, 1, 4, 0), (1, 0, 2, 2), (1, 65, 2, 2), (1, 1, 16384, 16384),
                             (200, 1, 1024, 1024)]):
        src = tmp_path / f"in{k}.bin"
        src.write_bytes(np.asarray(list(hdr) + [0, 0, 0, -1, 0, 1], np.int32).tobytes())
        assert subprocess.run([host_check, str(src), str(dst)], timeout=60).returncode == 3, hdr
    src = tmp_path / "markers.bin"
    src.write_bytes(np.asarray([1, 1, 2, 2, 0, 0, 0, -1, 257, 1], np.int32).tobytes())
    assert subprocess.run([host_check, str(src), str(dst)], timeout=60).returncode == 3


# ------------------------------------------------------------------------------------------------ the public function
@pytest.mark.parametrize("kind", ["point", "box", "mask"])
def test_numpy_path_equals_model_with_the_reference_selection(kind):
    frames, gt, outs, obj_to_cat = clip(6, 13, 17, 33, 5, kind, seed=3)
    sizes = set()
    for max_length, stride in [(4, 1), (4, 2), (4, 3), (2, 5), (8, 1), (8, 2), (1, 1), (5, 4)]:
        got = create_visualization_gif(frames, gt, outs, obj_to_cat, max_length=max_length, stride=stride,
                                       on_device=False)
        want = model_of_clip(frames, gt, outs, obj_to_cat, max_length, stride)
        assert got.dtype == np.uint8 and got.shape == want.shape == (want.shape[0], 3, 34, 66)
        assert np.array_equal(got, want), (kind, max_length, stride)
        sizes.add(got.shape[0])
    assert sizes == {1, 2, 3, 4, 5}  # 8 frames asked, 6 frames, 5 predictions: 5; stride > length: frame 0 alone
    got = create_visualization_gif(frames, gt, outs, obj_to_cat, on_device=False)  # the defaults: 4, 1
    assert np.array_equal(got, model_of_clip(frames, gt, outs, obj_to_cat, 4, 1))


def test_marker_table_and_palette():
    pal = V.category_palette(13)
    assert np.array_equal(pal, VC.palette_of(13)) and pal[0].tolist() == [229, 22, 22]
    _, _, outs, obj_to_cat = clip(2, 13, 17, 33, 2, "point")
    p = outs[0]["point_inputs"]
    assert V.prompt_type_of(p) == "point" and V.prompt_type_of(None) == "mask"
    got = V.prompt_markers(p, obj_to_cat, pal)
    assert np.array_equal(got, VC.markers_from_points(p["point_coords"].numpy(), p["point_labels"].numpy(), obj_to_cat, pal))
    assert len(got) == 9 and got.dtype == np.int32  # the three -1 paddings draw nothing
    neg = {"point_coords": torch.tensor([[[-0.7, 3.9]]]), "point_labels": torch.tensor([[1]])}
    assert V.prompt_markers(neg, [0], pal)[0, 1:3].tolist() == [0, 3]  # int() truncates towards zero
    _, _, outs, _ = clip(2, 13, 17, 33, 2, "box")
    assert V.prompt_type_of(outs[0]["point_inputs"]) == "bbox"
    many = {"point_coords": torch.zeros(300, 1, 2), "point_labels": torch.ones(300, 1, dtype=torch.int32)}
    with pytest.warns(UserWarning, match="300 prompt markers"):
        assert len(V.prompt_markers(many, [0] * 300, pal)) == 256


# ------------------------------------------------------------------------------------------------ the schedule
def _module(viz, **trainer):
    mod = SAM2LightningModule(SimpleNamespace(), {"iou_use_l1_loss": True, "weight_dict": {"loss_mask": 1, "loss_dice": 1, "loss_iou": 1}},
                              {"lr": 1e-4}, {"enabled": False}, viz)
    mod.trainer_ = SimpleNamespace(**{"is_global_zero": True, "current_epoch": 0, "batches_ready": 0, "global_step": 0,
                                      **trainer})
    return mod


def test_should_log_gif_truth_table():
    base = {"enabled": True, "train_every_n_steps": 20, "val_first_batch_every_n_epochs": 2}
    mod = _module(base)
    fired = []
    for ready in range(1, 61):
        mod.trainer_.batches_ready = ready
        if mod._should_log_gif("train", ready - 1):
            fired.append(ready)
    assert fired == [20, 40, 60]  # total.ready counts the current batch: 1 on the first
    for epoch, idx, want in [(0, 0, True), (0, 1, False), (1, 0, False), (2, 0, True), (3, 0, False), (4, 3, False)]:
        mod.trainer_.current_epoch = epoch
        assert mod._should_log_gif("val", idx) is want, (epoch, idx)
    assert mod._should_log_gif("test", 0) is False
    mod = _module(dict(base, train_every_n_steps=0, val_first_batch_every_n_epochs=0), current_epoch=3)
    for ready in (0, 1, 20):
        mod.trainer_.batches_ready = ready
        assert mod._should_log_gif("train", 0) is False  # steps = 0: never
    assert mod._should_log_gif("val", 0) is True and mod._should_log_gif("val", 1) is False  # epochs = 0: every epoch
    mod = _module(base, is_global_zero=False, batches_ready=20)
    assert mod._should_log_gif("train", 0) is False and mod._should_log_gif("val", 0) is False  # another rank
    for viz in (dict(base, enabled=False), None, {}):
        mod = _module(viz, batches_ready=20)
        assert mod._should_log_gif("train", 0) is False and mod._should_log_gif("val", 0) is False
    mod = _module(base, batches_ready=20)
    assert mod._should_log_gif("train", 0) is True
    assert mod._log_gif("train", None, None, None, None, "train") is None  # no save_dir: nothing is rendered
    assert mod.last_visualization is None


def test_trainer_counts_ready_batches():
    from sam2_video.training.trainer import Trainer
    assert Trainer().batches_ready == 0


# ------------------------------------------------------------------------------------------------ the writer
def test_save_visualization_round_trips(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(5)
    arr = rng.integers(0, 256, (3, 3, 10, 14), dtype=np.uint8)
    path = tmp_path / "sub" / "train_e0000_s0000002.gif"
    assert save_visualization(arr, path, fps=4, caption="run | train e0 s2") == [str(path)]
    with Image.open(path) as im:
        assert im.format == "GIF" and im.n_frames == 3 and im.size == (14, 10)
        assert im.info["loop"] == 0 and im.info["comment"] == b"run | train e0 s2"
        for i in range(3):
            im.seek(i)
            assert im.info["duration"] == 250
    save_visualization(torch.from_numpy(arr), tmp_path / "b.gif", fps=10)
    with Image.open(tmp_path / "b.gif") as im:
        assert im.info["duration"] == 100 and "comment" not in im.info
    files = save_visualization(arr, tmp_path / "c.gif", format="png")
    assert files == [str(tmp_path / f"c_f{i}.png") for i in range(3)]
    for i, f in enumerate(files):
        with Image.open(f) as im:
            assert np.array_equal(np.asarray(im.convert("RGB")), arr[i].transpose(1, 2, 0))
    assert save_visualization(arr[:0], tmp_path / "none.gif") == [] and not (tmp_path / "none.gif").exists()
    with pytest.raises(ValueError):
        save_visualization(arr.astype(np.float32), tmp_path / "d.gif")
    with pytest.raises(ValueError):
        save_visualization(arr, tmp_path / "d.webp", format="webp")


# ------------------------------------------------------------------------------------------------ the viewer
def test_viewer_host_path_equals_model(tmp_path):
    from PIL import Image
    from sam2_video.eval import visualize as VIS
    want = VC.build_viewer_tree(str(tmp_path))
    args = ["--gt", str(tmp_path / "gt.json"), "--predict", str(tmp_path / "predict.json"), "--image-root", str(tmp_path),
            "--host"]
    files = VIS.main(args + ["--prompt", str(tmp_path / "prompt.pkl"), "--out", str(tmp_path / "png"), "--format", "png"])
    assert sorted(os.path.basename(f) for f in files) == sorted(
        f"{name}_f{i}.png" for name, parts in want.items() for i in range(len(parts[0])))
    for name, parts in want.items():
        assert np.array_equal(VC.read_png_series(tmp_path / "png", name), VC.viewer_model(parts)), name
    # without prompt.pkl: whole videos, the first frame unmarked; GIF output, capped at two frames
    files = VIS.main(args + ["--out", str(tmp_path / "gif"), "--max-frames", "2"])
    assert sorted(os.path.basename(f) for f in files) == ["vidA_0.gif", "vidB_0.gif"]
    with Image.open(tmp_path / "gif" / "vidA_0.gif") as im:
        assert im.n_frames == 2 and im.size == (56, 40) and im.info["duration"] == 250
    with open(tmp_path / "gt.json") as f:
        coco = json.load(f)
    with open(tmp_path / "predict.json") as f:
        predict = json.load(f)
    vid_b = sorted((im for im in coco["images"] if im["video_id"] == "vidB"), key=lambda im: im["order_in_video"])
    whole = VIS.render_clip(vid_b, VIS._by_image(coco["annotations"]), VIS._by_image(predict), 4, None, str(tmp_path),
                            on_device=False)
    frames, _, gt, pr, _, _ = want["vidB_0"]
    assert np.array_equal(whole, VC.viewer_model((frames, frames[0], gt, pr, None, None)))
