"""Clip loading on the device (data section `preprocess_on_device: true`).

The DataLoader workers stop after the image decode: an item of data/dataset.py is then the uint8 frames and
the annotations' COCO RLE run boundaries.  `sam2_raw_collate_fn` packs a clip into a `RawVideoDatapoint`
(frames of one size stacked, their runs back to back with a CSR over the frames), which is pinned and copied
like a batch -- 3.9 MB per 1024 x 1280 frame and a few KB of runs instead of the finished fp32 images and bool
masks -- and `DeviceClipPreprocessor` turns it into the `BatchedVideoDatapoint` the step reads:
`ops.resample_u8_norm` (Pillow's fixed-point bilinear resize, center crop, normalisation) and
`ops.rle_catmasks` (nearest resize, center crop and the per-category OR straight from the runs), the same
tensors as `sam2_collate_fn` on the host items, bit for bit.  Frame 0's dense masks travel along on the host
(`masks0` -> `host_masks0`): the prompt stage samples its clicks from them without waiting for the device.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List

import torch

from .data_utils import BatchedVideoDatapoint, BatchedVideoMetaData
from .dataset import IMAGENET_MEAN, IMAGENET_STD, center_crop_box, resized_hw


@dataclass
class RawFrameGroup:
    """the frames of one size of a clip: frame_idx int64 [F] (their positions in the clip), frames uint8
    [F, H, W, 3], and their annotations back to back: run_off int32 [A + 1], run_end int32 [R], ann_cat int32
    [A], frame_off int32 [F + 1] (ops.rle_catmasks)"""
    frame_idx: torch.Tensor
    frames: torch.Tensor
    run_off: torch.Tensor
    run_end: torch.Tensor
    ann_cat: torch.Tensor
    frame_off: torch.Tensor

    def _map(self, fn):
        return RawFrameGroup(frame_idx=self.frame_idx, frames=fn(self.frames), run_off=fn(self.run_off),
                             run_end=fn(self.run_end), ann_cat=fn(self.ann_cat), frame_off=fn(self.frame_off))


@dataclass
class RawVideoDatapoint:
    """a clip before preprocessing: `groups` cover its `num_frames` frames once each; masks0 bool [N, S, S] =
    frame 0's category masks, host-side, never copied to the device"""
    groups: List[RawFrameGroup]
    masks0: torch.Tensor
    num_frames: int
    dict_key: str = "video_batch"

    @property
    def num_categories(self) -> int:
        return int(self.masks0.shape[0])

    @property
    def image_size(self) -> int:
        return int(self.masks0.shape[-1])

    def to(self, device, non_blocking=False):
        return RawVideoDatapoint(groups=[g._map(lambda t: t.to(device, non_blocking=non_blocking))
                                         for g in self.groups],
                                 masks0=self.masks0, num_frames=self.num_frames, dict_key=self.dict_key)

    def pin_memory(self, device=None):
        return RawVideoDatapoint(groups=[g._map(lambda t: t.pin_memory()) for g in self.groups],
                                 masks0=self.masks0, num_frames=self.num_frames, dict_key=self.dict_key)


def sam2_raw_collate_fn(batch_list):
    """[{"frames": T x uint8 [H, W, 3], "runs": T x (run_off, run_end, ann_cat), "masks0": [N, S, S] bool}] ->
    RawVideoDatapoint (B must be 1, as sam2_collate_fn)"""
    assert len(batch_list) == 1, f"Only batch_size=1 is supported in the simplified pipeline, got B={len(batch_list)}"
    item = batch_list[0]
    frames, runs = item["frames"], item["runs"]
    by_size = {}
    for t, f in enumerate(frames):
        by_size.setdefault(tuple(f.shape[:2]), []).append(t)
    groups = []
    for idx in by_size.values():
        offs, ends, cats, foff, base = [torch.zeros(1, dtype=torch.int32)], [], [], [0], 0
        for t in idx:
            run_off, run_end, ann_cat = runs[t]
            offs.append(run_off[1:] + base)
            ends.append(run_end)
            cats.append(ann_cat)
            base += int(run_end.numel())
            foff.append(foff[-1] + int(ann_cat.numel()))
        groups.append(RawFrameGroup(frame_idx=torch.tensor(idx, dtype=torch.long),
                                    frames=torch.stack([frames[t] for t in idx]),
                                    run_off=torch.cat(offs).to(torch.int32), run_end=torch.cat(ends).to(torch.int32),
                                    ann_cat=torch.cat(cats).to(torch.int32),
                                    frame_off=torch.tensor(foff, dtype=torch.int32)))
    return RawVideoDatapoint(groups=groups, masks0=item["masks0"].bool(), num_frames=len(frames))


class DeviceClipPreprocessor:
    """RawVideoDatapoint -> BatchedVideoDatapoint on the device, `host_masks0` set: the tensors of
    `sam2_collate_fn(host items).to(device)`.  HIP kernels on the current stream; no device -> host copy."""

    def __init__(self, image_size: int, num_categories: int, mean=IMAGENET_MEAN, std=IMAGENET_STD):
        self.image_size, self.num_categories = int(image_size), int(num_categories)
        self.mean, self.std = tuple(mean), tuple(std)
        self._maps = {}

    def _nearest_maps(self, H, W, device):
        key = (H, W, str(device))
        m = self._maps.get(key)
        if m is None:
            from ..kernels import ops
            m = self._maps[key] = tuple(torch.from_numpy(a.copy()).to(device)
                                        for a in ops.nearest_maps(H, W, self.image_size))
        return m

    def __call__(self, raw: RawVideoDatapoint, device="cuda", non_blocking: bool = True) -> BatchedVideoDatapoint:
        from ..kernels import ops
        S, N, T = self.image_size, self.num_categories, raw.num_frames
        if raw.num_categories != N or raw.image_size != S:
            raise ValueError(f"clip of {raw.num_categories} categories at {raw.image_size}, preprocessor built "
                             f"for {N} at {S}")
        device = torch.device(device)
        raw = raw.to(device, non_blocking=non_blocking)
        whole = len(raw.groups) == 1 and raw.groups[0].frame_idx.tolist() == list(range(T))
        images = torch.empty(T, 3, S, S, device=device, dtype=torch.float32)
        masks = torch.empty(T, N, S, S, device=device, dtype=torch.bool)
        seen = 0
        for g in raw.groups:
            F, H, W, _ = g.frames.shape
            nh, nw = resized_hw(H, W, S)
            img = ops.resample_u8_norm(g.frames, (nh, nw), center_crop_box(nh, nw, S, S), "bilinear", self.mean,
                                       self.std, crop_hw=(S, S), out=images if whole else None)
            rows, cols = self._nearest_maps(H, W, device)
            msk = ops.rle_catmasks(g.run_off, g.run_end, g.ann_cat, g.frame_off, H, W, rows, cols, N,
                                   out=masks if whole else None)
            if not whole:
                at = g.frame_idx.to(device)
                images[at] = img
                masks[at] = msk
            seen += F
        if seen != T:
            raise ValueError(f"the groups hold {seen} frames, the clip has {T}")
        t_idx = torch.arange(T, dtype=torch.int32, device=device).view(T, 1).expand(T, N)
        obj_to_frame_idx = torch.stack([t_idx, torch.zeros_like(t_idx)], dim=-1).contiguous()
        n_idx = torch.arange(N, dtype=torch.long, device=device).view(1, N).expand(T, N)
        ident = torch.stack([torch.zeros_like(n_idx), n_idx,
                             torch.arange(T, dtype=torch.long, device=device).view(T, 1).expand(T, N)],
                            dim=-1).contiguous()
        orig = torch.full((T, N, 2), fill_value=S, dtype=torch.long, device=device)
        meta = BatchedVideoMetaData(unique_objects_identifier=ident, frame_orig_size=orig)
        out = BatchedVideoDatapoint(img_batch=images.view(T, 1, 3, S, S), obj_to_frame_idx=obj_to_frame_idx, masks=masks,
                                    metadata=meta, dict_key=raw.dict_key, batch_size=[T])
        out.host_masks0 = raw.masks0
        return out


_PREPROCESSORS = {}


def to_device_batch(batch, device, non_blocking: bool = True):
    """what the trainer does with a loader's batch: a RawVideoDatapoint goes through the device preprocessor
    (one per clip geometry), anything else is copied as before"""
    if isinstance(batch, RawVideoDatapoint):
        key = (batch.image_size, batch.num_categories)
        pre = _PREPROCESSORS.get(key)
        if pre is None:
            pre = _PREPROCESSORS[key] = DeviceClipPreprocessor(*key)
        return pre(batch, device, non_blocking=non_blocking)
    return batch.to(device, non_blocking=non_blocking)
