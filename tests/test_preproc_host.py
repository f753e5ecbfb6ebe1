"""Clip loading on the device, the parts that need no GPU: ops.resample_taps against Pillow itself, the shared
header of csrc/preproc.hip compiled for the host and run in the kernels' decomposition
(csrc/preproc_host_check.cpp, also under the address and undefined-behaviour sanitizers, as a program) against
Pillow and dataset.resize_mask(rle.decode(.)), rle.runs_hit_grid against dense masks, the raw dataset items and
their collate."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import preproc_cases as C
from sam2_video.data import dataset as D
from sam2_video.data import rle
from sam2_video.kernels import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sam2-video-training_amd", "csrc")
PIL_FILTER = {"bilinear": "BILINEAR", "bicubic": "BICUBIC"}


def _pil_resize(arr, nh, nw, filt=None):
    from PIL import Image
    img = Image.fromarray(arr)
    return np.asarray(img.resize((nw, nh)) if filt is None else img.resize((nw, nh), getattr(Image, PIL_FILTER[filt])))


# --------------------------------------------------------------------------------------------------- the taps
@pytest.mark.parametrize("filt", ["bilinear", "bicubic"])
@pytest.mark.parametrize("shape", C.RESIZE_SHAPES, ids=lambda s: f"{s[0][0]}x{s[0][1]}to{s[1][0]}x{s[1][1]}")
def test_taps_reproduce_pillow(shape, filt):
    (H, W), (nh, nw) = shape
    for kind in ("random", "smooth"):
        arr = C.test_image(H, W, kind, seed=H + nw)
        want = _pil_resize(arr, nh, nw, filt)
        got = C.model_resize(arr, nh, nw, filt)
        assert int((want != got).sum()) == 0, f"{kind}: {int((want != got).sum())} bytes differ"


def test_pillow_default_filter_is_bicubic():
    """predictor._load_frames calls Image.resize without a filter: the device path uses the bicubic taps"""
    for (H, W), (nh, nw) in C.RESIZE_SHAPES[:4]:
        arr = C.test_image(H, W, "random", seed=3)
        assert np.array_equal(_pil_resize(arr, nh, nw), _pil_resize(arr, nh, nw, "bicubic"))
        assert np.array_equal(_pil_resize(arr, nh, nw), C.model_resize(arr, nh, nw, "bicubic"))


def test_taps_layout_and_cache():
    xmin, cnt, coef = ops.resample_taps(53, 22, "bilinear")
    assert xmin.dtype == cnt.dtype == coef.dtype == np.int32 and coef.shape == (22, coef.shape[1])
    assert (xmin >= 0).all() and (cnt >= 1).all() and (xmin + cnt <= 53).all() and (cnt <= coef.shape[1]).all()
    assert all((coef[o, cnt[o]:] == 0).all() for o in range(22))
    assert abs(int(coef.sum(1).max()) - (1 << 22)) <= coef.shape[1]  # the weights are normalised
    assert ops.resample_taps(53, 22, "bilinear")[2] is coef
    ident = ops.resample_taps(17, 17, "bicubic")  # an unchanged axis: Pillow skips the pass, these taps copy
    assert np.array_equal(C.model_axis(np.arange(17, dtype=np.uint8)[:, None] * 15, ident, 0)[:, 0],
                          np.arange(17, dtype=np.uint8) * 15)
    with pytest.raises(ValueError):
        ops.resample_taps(8, 8, "lanczos")


def test_norm_lut_is_the_loaders_expression():
    lut = ops.norm_lut(D.IMAGENET_MEAN, D.IMAGENET_STD)
    v = torch.arange(256, dtype=torch.uint8).view(1, 16, 16).expand(3, 16, 16)
    x = v.float() / 255.0
    want = (x - torch.tensor(D.IMAGENET_MEAN).view(3, 1, 1)) / torch.tensor(D.IMAGENET_STD).view(3, 1, 1)
    assert torch.equal(lut, want.reshape(3, 256))


# ------------------------------------------------------------------------------------------------ the header
@pytest.fixture(scope="module", params=["plain", "sanitized"])
def host_check(request, tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build csrc/preproc_host_check.cpp")
    exe = tmp_path_factory.mktemp("pp_host") / f"preproc_host_check_{request.param}"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", *flags, "-I", CSRC,
                    os.path.join(CSRC, "preproc_host_check.cpp"), "-o", str(exe)], check=True)
    return str(exe)


def _run(exe, tmp_path, cases):
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    C.write_cases(src, cases)
    subprocess.run([exe, str(src), str(dst)], check=True, timeout=300)
    return dst.read_bytes()


def _norm(u8_hwc):
    """[.., h, w, 3] uint8 -> [.., 3, h, w] fp32 as load_image normalises"""
    x = torch.from_numpy(np.ascontiguousarray(u8_hwc)).movedim(-1, -3).float().div_(255.0)
    return (x - torch.tensor(D.IMAGENET_MEAN).view(3, 1, 1)) / torch.tensor(D.IMAGENET_STD).view(3, 1, 1)


def test_header_resample(host_check, tmp_path):
    lut = ops.norm_lut(D.IMAGENET_MEAN, D.IMAGENET_STD).numpy()
    shapes = C.RESIZE_SHAPES[:4] if host_check.endswith("sanitized") else C.RESIZE_SHAPES
    cases, want = [], []
    for (H, W), (nh, nw) in shapes:
        for filt in ("bilinear", "bicubic"):
            frames = np.stack([C.test_image(H, W, "random", seed=1), C.test_image(H, W, "smooth")])
            if H >= 1024:
                frames = frames[:1]
            # the whole image, and a window off the borders (the horizontal pass then skips source rows)
            top, left = nh // 4, nw // 3
            for (t, l), (ch, cw) in (((0, 0), (nh, nw)), ((top, left), (nh - top - 1, nw - left - 2))):
                cases.append(C.resample_case(frames, (nh, nw), (t, l), (ch, cw), filt, lut))
                full = np.stack([_pil_resize(f, nh, nw, filt) for f in frames])
                want.append(_norm(full[:, t:t + ch, l:l + cw]).numpy())
    raw = np.frombuffer(_run(host_check, tmp_path, cases), np.float32)
    off = 0
    for w in want:
        assert np.array_equal(raw[off:off + w.size].view(np.int32), w.reshape(-1).view(np.int32))
        off += w.size
    assert off == raw.size


def test_header_damaged_tables_stay_inside(host_check, tmp_path):
    """tap windows that leave the line or overrun their table row are cut, not followed (the sanitizers watch)"""
    lut = ops.norm_lut(D.IMAGENET_MEAN, D.IMAGENET_STD).numpy()
    frames = C.test_image(9, 11, "random")[None]
    hdr, arrays = C.resample_case(frames, (5, 6), (0, 0), (5, 6), "bilinear", lut)
    arrays = [np.array(a) for a in arrays]
    arrays[1][:] = [-3, 0, 9, 10, 11, 400]      # x_min
    arrays[2][:] = [5, 100, 4, 1, 1, 1]         # x_cnt
    arrays[4][:] = [-2, 0, 7, 8, 9]             # y_min
    arrays[5][:] = [3, 77, 5, 1, 1]             # y_cnt
    raw = np.frombuffer(_run(host_check, tmp_path, [(hdr, arrays)]), np.float32)
    assert raw.size == 3 * 5 * 6 and np.isfinite(raw).all()


@pytest.mark.parametrize("H,W,S,N", [(40, 56, 32, 4), (23, 19, 16, 13), (8, 8, 16, 64), (61, 37, 24, 13)])
def test_header_catmasks(host_check, tmp_path, H, W, S, N):
    frames = C.catmask_frames(H, W, N)
    run_off, run_end, ann_cat, frame_off = C.runs_of(frames, H, W)
    rows, cols = ops.nearest_maps(H, W, S)
    hdr = (1, len(frames), N, H, W, ann_cat.size, run_end.size, S, S)
    raw = np.frombuffer(_run(host_check, tmp_path, [(hdr, [run_off, run_end, ann_cat, frame_off, rows, cols])]),
                        np.uint8)
    want = C.dense_catmasks(frames, N, S).numpy().astype(np.uint8)
    assert raw.size == want.size and np.array_equal(raw.reshape(want.shape), want)
    assert want.any() and not want.all()


def test_nearest_maps_are_resize_mask():
    for H, W, S in ((40, 56, 32), (56, 40, 32), (23, 19, 16), (8, 8, 16), (1024, 1280, 512)):
        rows, cols = ops.nearest_maps(H, W, S)
        idx = np.arange(H * W, dtype=np.float32).reshape(H, W)  # (exact in fp32 up to 2^24)
        nh, nw = D.resized_hw(H, W, S)
        t = torch.nn.functional.interpolate(torch.from_numpy(idx)[None, None], size=(nh, nw), mode="nearest")[0, 0]
        top, left = D.center_crop_box(nh, nw, S, S)
        assert np.array_equal(t[top:top + S, left:left + S].numpy(), idx[rows][:, cols])


# ------------------------------------------------------------------------------------------- runs_hit_grid
def _hit_cases(H, W, S):
    rows, cols = ops.nearest_maps(H, W, S)
    on_r, on_c = int(rows[S // 2]), int(cols[S // 3])
    off_r = next(r for r in range(H) if r not in set(rows.tolist()))
    z = np.zeros((H, W), np.uint8)
    margin = z.copy()  # the long side loses its ends to the center crop
    if W > H:
        margin[:, :cols.min()] = 1
        margin[:, cols.max() + 1:] = 1
    else:
        margin[:rows.min(), :] = 1
        margin[rows.max() + 1:, :] = 1
    assert margin.any()
    cases = {"empty": z.copy(), "full": np.ones((H, W), np.uint8)}
    cases["one pixel on the grid"] = z.copy()
    cases["one pixel on the grid"][on_r, on_c] = 1
    cases["one pixel off the grid"] = z.copy()
    cases["one pixel off the grid"][off_r, on_c] = 1
    cases["run across two columns"] = z.copy()
    cases["run across two columns"][H - 2:, on_c] = 1
    cases["run across two columns"][:2, on_c + 1] = 1
    cases["only the cropped margin"] = margin
    cases["first pixel only"] = z.copy()
    cases["first pixel only"][0, 0] = 1
    cases["last pixel only"] = z.copy()
    cases["last pixel only"][H - 1, W - 1] = 1
    return rows, cols, cases


@pytest.mark.parametrize("H,W,S", [(40, 72, 16), (72, 40, 16), (37, 53, 8)])
def test_runs_hit_grid_is_the_dense_answer(H, W, S):
    rows, cols, cases = _hit_cases(H, W, S)
    rng = np.random.default_rng(5)
    for k in range(6):  # sparse random masks: some hit, some miss
        m = np.zeros((H, W), np.uint8)
        m[rng.integers(0, H, 2), rng.integers(0, W, 2)] = 1
        cases[f"random {k}"] = m
    answers = set()
    for name, m in cases.items():
        counts = rle.counts_from_string(rle.encode(m)["counts"])
        _, run_end = ops.rle_runs([counts], H, W)
        want = bool(D.resize_mask(rle.decode(rle.encode(m)), S).any())
        assert rle.runs_hit_grid(run_end, H, rows, cols) == want, name
        answers.add(want)
    assert not D.resize_mask(cases["only the cropped margin"], S).any()
    assert not D.resize_mask(cases["one pixel off the grid"], S).any()
    assert answers == {True, False}


# ---------------------------------------------------------------------------------- raw dataset and collate
def test_raw_items_and_collate(tmp_path):
    from PIL import Image
    from sam2_video.data.preprocess import RawVideoDatapoint, sam2_raw_collate_fn
    T, H, W, N, S = 4, 40, 56, 4, 32
    _, cfg = C.write_coco(str(tmp_path), T, H, W, N, S, empty=(1,), clip=3)
    host = D.COCODataset(config=cfg)
    raw = D.COCODataset(config=dict(cfg, preprocess_on_device=True))
    assert not host.video_dataset.image_dataset.preprocess_on_device
    assert len(raw) == len(host) == 2
    ids, rids = host.video_dataset.image_dataset, raw.video_dataset.image_dataset
    # the empty-image replacement picks the same index: image 1 has no annotation, image 2 stands in
    assert rids[1]["index"] == 2 and torch.equal(ids[1]["masks"], ids[2]["masks"])
    for i in range(T):
        item = rids[i]
        j = item["index"]
        assert torch.equal(ids[i]["masks"], ids._load_gt_masks_for_image(ids.images[j]["id"]))
        frame = np.asarray(Image.open(ids.images[j]["path"]).convert("RGB"))
        assert item["frame"].dtype == torch.uint8 and np.array_equal(item["frame"].numpy(), frame)
        run_off, run_end, ann_cat = item["runs"]
        anns = [a for a in ids.image_id_to_annotations[ids.images[j]["id"]] if a["category_id"] in ids.catid_to_idx]
        assert ann_cat.tolist() == [ids.catid_to_idx[a["category_id"]] for a in anns]
        for k, a in enumerate(anns):
            counts = rle.counts_from_string(a["segmentation"]["counts"])
            assert run_end[run_off[k]:run_off[k + 1]].tolist() == np.cumsum(counts).tolist()
    assert not rids.mask_cache  # the runs are cached, no dense mask
    clip, hclip = raw[0], host[0]
    assert len(clip["frames"]) == 3 and torch.equal(clip["masks0"], hclip["masks"][0])
    assert not rids.mask_cache
    dp = sam2_raw_collate_fn([clip])
    assert isinstance(dp, RawVideoDatapoint) and dp.num_frames == 3 and dp.image_size == S and dp.num_categories == N
    assert len(dp.groups) == 1
    g = dp.groups[0]
    assert g.frames.shape == (3, H, W, 3) and g.frame_idx.tolist() == [0, 1, 2]
    assert g.frame_off.tolist() == np.cumsum([0] + [r[2].numel() for r in clip["runs"]]).tolist()
    assert g.run_off.tolist() == np.cumsum([0] + [n for r in clip["runs"] for n in np.diff(r[0].numpy())]).tolist()
    assert torch.equal(g.run_end, torch.cat([r[1] for r in clip["runs"]]))
    moved = dp.to("cpu")
    assert torch.equal(moved.groups[0].frames, g.frames) and moved.masks0 is dp.masks0
    # host model of the preprocessor: the groups rebuild the host clip's masks
    rows, cols = ops.nearest_maps(H, W, S)
    for f in range(3):
        dense = torch.zeros(N, S, S, dtype=torch.bool)
        for a in range(int(g.frame_off[f]), int(g.frame_off[f + 1])):
            ends = g.run_end[int(g.run_off[a]):int(g.run_off[a + 1])].numpy()
            pos = cols[None, :].astype(np.int64) * H + rows[:, None]
            dense[int(g.ann_cat[a])] |= torch.from_numpy((np.searchsorted(ends, pos, side="right") & 1).astype(bool))
        assert torch.equal(dense, hclip["masks"][f])


def test_collate_groups_frames_by_size():
    from sam2_video.data.preprocess import sam2_raw_collate_fn
    def item(h, w, n_ann):
        counts = [[h * w - 3, 3]] * n_ann
        off, end = ops.rle_runs(counts, h, w)
        return torch.zeros(h, w, 3, dtype=torch.uint8), (torch.from_numpy(off), torch.from_numpy(end),
                                                         torch.arange(n_ann, dtype=torch.int32))
    items = [item(8, 10, 1), item(6, 6, 2), item(8, 10, 3)]
    dp = sam2_raw_collate_fn([{"frames": [i[0] for i in items], "runs": [i[1] for i in items],
                               "masks0": torch.zeros(3, 4, 4, dtype=torch.bool)}])
    assert [g.frame_idx.tolist() for g in dp.groups] == [[0, 2], [1]]
    assert dp.groups[0].frame_off.tolist() == [0, 1, 4] and dp.groups[0].run_off.tolist() == [0, 2, 4, 6, 8]
    assert dp.groups[1].frames.shape == (2 - 1, 6, 6, 3) and dp.groups[1].ann_cat.tolist() == [0, 1]


def test_binding_declares_the_loader_entry_points():
    from sam2_video.kernels import _lib
    assert len(_lib.SIGNATURES["s2h_resample_u8_norm"]) == 20 and len(_lib.SIGNATURES["s2h_rle_catmasks"]) == 15
