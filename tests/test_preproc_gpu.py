"""Clip loading on the device (csrc/preproc.hip) against the host loaders it replaces, bit for bit:
ops.resample_u8_norm against dataset.load_image and predictor._load_frames on files written by PIL,
ops.rle_catmasks against COCOImageDataset._load_gt_masks_for_image's computation, DeviceClipPreprocessor against
sam2_collate_fn(host items).to("cuda"), one training step's loss from the host loader and from the device
loader, and the predictor's init_state / first propagated frame with preprocess_on_device on and off."""
import os

import numpy as np
import pytest
import torch

import preproc_cases as C
from sam2_video.data import dataset as D

pytestmark = pytest.mark.gpu


def _save(arr, path):
    from PIL import Image
    Image.fromarray(arr).save(path)
    return str(path)


def _device_load_image(frames_u8, S):
    """dataset.load_image's geometry through the kernel"""
    from sam2_video.kernels import ops
    _, H, W, _ = frames_u8.shape
    nh, nw = D.resized_hw(H, W, S)
    return ops.resample_u8_norm(frames_u8.cuda(), (nh, nw), D.center_crop_box(nh, nw, S, S), "bilinear",
                                D.IMAGENET_MEAN, D.IMAGENET_STD, crop_hw=(S, S))


# ------------------------------------------------------------------------------------------ resample_u8_norm
@pytest.mark.parametrize("H,W,S,F", [(37, 53, 16, 1), (19, 23, 32, 1), (53, 37, 16, 1), (1024, 1280, 512, 1),
                                     (40, 56, 32, 2)])
def test_resample_equals_load_image(tmp_path, H, W, S, F):
    frames = np.stack([C.test_image(H, W, "smooth" if f else "random", seed=S + f) for f in range(F)])
    want = torch.stack([D.load_image(_save(frames[f], tmp_path / f"{f}.png"), S) for f in range(F)])
    got = _device_load_image(torch.from_numpy(frames), S)
    assert got.shape == (F, 3, S, S) and got.dtype == torch.float32
    assert torch.equal(got.cpu(), want)


@pytest.mark.parametrize("H,W,S", [(37, 53, 16), (19, 23, 32), (64, 64, 64), (150, 200, 128)])
def test_resample_bicubic_equals_load_frames(tmp_path, H, W, S):
    from sam2_video.kernels import ops
    from sam2_video.predictor import _load_frames, _load_frames_device
    frames = np.stack([C.test_image(H, W, "random", seed=1), C.test_image(H, W, "smooth"),
                       C.test_image(H, W, "random", seed=2)])
    want, vh, vw = _load_frames(frames, S)
    got = ops.resample_u8_norm(torch.from_numpy(frames).cuda(), (S, S), (0, 0), "bicubic")
    assert (vh, vw) == (H, W) and torch.equal(got.cpu(), want)
    # a JPEG folder, in chunks that do not divide the frame count, on the device and copied back
    for f in range(3):
        from PIL import Image
        Image.fromarray(frames[f]).save(tmp_path / f"{f}.jpg", quality=90)
    want, vh, vw = _load_frames(str(tmp_path), S)
    for keep in (True, False):
        got, gh, gw = _load_frames_device(str(tmp_path), S, torch.device("cuda"), 2, keep_on_device=keep)
        assert (gh, gw) == (vh, vw) == (H, W) and got.is_cuda == keep and torch.equal(got.cpu(), want)


def test_resample_rejects_what_it_cannot_index():
    from sam2_video.kernels import ops
    from sam2_video.kernels._lib import HipKernelError, lib
    x = torch.zeros(1, 8, 2000, 3, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="taps"):
        ops.resample_u8_norm(x, (8, 16), (0, 0), "bicubic")  # a down-scale by 125: more than 64 taps
    with pytest.raises(ValueError, match="outside"):
        ops.resample_u8_norm(x, (8, 100), (0, 90), "bilinear", crop_hw=(8, 16))
    z = torch.zeros(64, dtype=torch.int32, device="cuda")
    assert lib().s2h_resample_u8_norm(1, 8, 8, x.data_ptr(), 4, 65, z.data_ptr(), z.data_ptr(), z.data_ptr(), 4, 3,
                                      z.data_ptr(), z.data_ptr(), z.data_ptr(), 0, 8, z.data_ptr(), x.data_ptr(),
                                      z.data_ptr(), None) != 0
    assert issubclass(HipKernelError, RuntimeError)


# ---------------------------------------------------------------------------------------------- rle_catmasks
@pytest.mark.parametrize("H,W,S,N", [(40, 56, 32, 4), (23, 19, 16, 13), (8, 8, 16, 64), (150, 200, 128, 13)])
def test_catmasks_equal_the_dense_path(H, W, S, N):
    from sam2_video.kernels import ops
    frames = C.catmask_frames(H, W, N)
    assert len(frames[0]) != len(frames[1])
    run_off, run_end, ann_cat, frame_off = C.runs_of(frames, H, W)
    rows, cols = ops.nearest_maps(H, W, S)
    dev = [torch.from_numpy(np.array(a)).cuda() for a in (run_off, run_end, ann_cat, frame_off, rows, cols)]
    got = ops.rle_catmasks(*dev[:4], H, W, dev[4], dev[5], N)
    want = C.dense_catmasks(frames, N, S)
    assert got.dtype == torch.bool and got.shape == want.shape
    assert torch.equal(got.cpu(), want)
    assert want[0, 0].any() and not want[0, 1].any()  # category 1 has no annotation
    # every element is written: a second call into a dirty buffer gives the same
    dirty = torch.full_like(got, True)
    assert torch.equal(ops.rle_catmasks(*dev[:4], H, W, dev[4], dev[5], N, out=dirty).cpu(), want)


def test_catmasks_equal_the_dataset(tmp_path):
    """the dataset's own annotations (an unknown category id skipped, several annotations per image)"""
    from sam2_video.kernels import ops
    T, H, W, N, S = 3, 40, 56, 4, 32
    _, cfg = C.write_coco(str(tmp_path), T, H, W, N, S)
    host = D.COCOImageDataset(cfg)
    raw = D.COCOImageDataset(dict(cfg, preprocess_on_device=True))
    rows, cols = (torch.from_numpy(a.copy()).cuda() for a in ops.nearest_maps(H, W, S))
    for i in range(T):
        run_off, run_end, ann_cat = raw[i]["runs"]
        foff = torch.tensor([0, ann_cat.numel()], dtype=torch.int32)
        got = ops.rle_catmasks(run_off.cuda(), run_end.cuda(), ann_cat.cuda(), foff.cuda(), H, W, rows, cols, N)
        assert torch.equal(got[0].cpu(), host._load_gt_masks_for_image(host.images[i]["id"]))


# ---------------------------------------------------------------------------------------------- preprocessor
def _same_batch(a, b):
    for name in ("img_batch", "obj_to_frame_idx", "masks"):
        x, y = getattr(a, name), getattr(b, name)
        assert x.dtype == y.dtype and x.device == y.device and torch.equal(x, y), name
    for name in ("unique_objects_identifier", "frame_orig_size"):
        x, y = getattr(a.metadata, name), getattr(b.metadata, name)
        assert x.dtype == y.dtype and x.device == y.device and torch.equal(x, y), name
    assert a.batch_size == b.batch_size and a.dict_key == b.dict_key
    assert not a.host_masks0.is_cuda and torch.equal(a.host_masks0, b.host_masks0)


def test_preprocessor_equals_host_collate(tmp_path):
    from sam2_video.data.preprocess import DeviceClipPreprocessor, sam2_raw_collate_fn
    from sam2_video.data.synthetic import sam2_collate_fn
    T, N, S, H, W = 3, 4, 32, 40, 56
    _, cfg = C.write_coco(str(tmp_path), T, H, W, N, S)
    host = D.COCODataset(config=cfg)
    raw = D.COCODataset(config=dict(cfg, preprocess_on_device=True))
    want = sam2_collate_fn([host[0]]).to("cuda")
    got = DeviceClipPreprocessor(S, N)(sam2_raw_collate_fn([raw[0]]).pin_memory())
    assert got.img_batch.shape == (T, 1, 3, S, S) and got.masks.shape == (T, N, S, S)
    _same_batch(got, want)


def test_preprocessor_groups_frames_of_different_sizes(tmp_path):
    from sam2_video.data.preprocess import DeviceClipPreprocessor, sam2_raw_collate_fn
    from sam2_video.data.synthetic import sam2_collate_fn
    N, S = 3, 16
    _, a = C.write_coco(str(tmp_path / "a"), 2, 40, 56, N, S, seed=1)
    _, b = C.write_coco(str(tmp_path / "b"), 2, 37, 23, N, S, seed=2)
    ha, hb = D.COCODataset(config=a)[0], D.COCODataset(config=b)[0]
    ra, rb = (D.COCODataset(config=dict(c, preprocess_on_device=True))[0] for c in (a, b))
    order = [(0, 0), (1, 0), (0, 1)]  # (set, frame): sizes interleaved
    hs, rs = (ha, hb), (ra, rb)
    host = {"images": torch.stack([hs[s]["images"][f] for s, f in order]),
            "masks": torch.stack([hs[s]["masks"][f] for s, f in order])}
    raw = {"frames": [rs[s]["frames"][f] for s, f in order], "runs": [rs[s]["runs"][f] for s, f in order],
           "masks0": ra["masks0"]}
    dp = sam2_raw_collate_fn([raw])
    assert [g.frame_idx.tolist() for g in dp.groups] == [[0, 2], [1]]
    _same_batch(DeviceClipPreprocessor(S, N)(dp), sam2_collate_fn([host]).to("cuda"))


# --------------------------------------------------------------------------------------------- training step
def test_training_loss_is_the_same_from_both_loaders(tmp_path):
    from step_harness import ALL, build_model
    from test_training_step_gpu import make_module, step
    from sam2_video.data.preprocess import RawVideoDatapoint
    from sam2_video.training.trainer import SAM2LightningDataModule, _to_device
    N, S = 3, 256
    path, _ = C.write_coco(str(tmp_path), 2, 72, 96, N, S)
    data = {"train_path": path, "val_path": path, "image_size": S, "video_clip_length": 2, "stride": 1,
            "num_categories": N, "batch_size": 1, "num_workers": 0}
    batches = []
    for flag in (False, True):
        dm = SAM2LightningDataModule(dict(data, preprocess_on_device=flag), train_shuffle=False)
        dm.setup("fit")
        batch = next(iter(dm.train_dataloader()))
        assert isinstance(batch, RawVideoDatapoint) == flag
        batches.append(_to_device(batch, torch.device("cuda")))
    assert torch.equal(batches[0].img_batch, batches[1].img_batch) and torch.equal(batches[0].masks, batches[1].masks)
    assert bool(batches[0].masks[0].any())
    model = build_model("tiny", S, ALL, "point", dtype="fp32", seed=0)
    sec = {"gt_stride": 1, "weight_dict": {"loss_mask": 20, "loss_dice": 1, "loss_iou": 1, "loss_class": 0},
           "supervise_all_iou": True, "iou_use_l1_loss": True}
    mod = make_module(model, sec)
    losses = [float(step(mod, b).detach()) for b in batches]
    print("loss host loader, device loader:", losses)
    assert np.isfinite(losses[0]) and losses[0] == losses[1]


# ------------------------------------------------------------------------------------------------- predictor
def test_predictor_init_state_and_first_frame(tmp_path):
    from step_harness import ALL, build_model
    from sam2_video.predictor import SAM2VideoPredictor
    S = 256
    video = np.stack([C.test_image(64, 96, "smooth"), C.test_image(64, 96, "random", seed=4),
                      C.test_image(64, 96, "smooth", seed=1)])
    model = build_model("tiny", S, ALL, "point", dtype="fp32", seed=0)
    first = []
    for flag in (False, True):
        pred = SAM2VideoPredictor(model, preprocess_on_device=flag, frame_chunk=2)
        st = pred.init_state(video)
        assert st["images"].is_cuda and (st["video_height"], st["video_width"]) == (64, 96)
        pred.add_new_points_or_box(st, 0, obj_id=1, points=[[40.0, 30.0]], labels=[1])
        t, ids, vm = next(iter(pred.propagate_in_video(st)))
        first.append((st["images"].clone(), t, vm.clone()))
        off = pred.init_state(video, offload_video_to_cpu=True)
        assert not off["images"].is_cuda and torch.equal(off["images"], st["images"].cpu())
    assert torch.equal(first[0][0], first[1][0])
    assert first[0][1] == first[1][1] == 0 and torch.equal(first[0][2], first[1][2])
    # a floating-point input passes through as before
    pred = SAM2VideoPredictor(model, preprocess_on_device=True)
    assert torch.equal(pred.init_state(first[0][0].cpu())["images"], first[0][0])
