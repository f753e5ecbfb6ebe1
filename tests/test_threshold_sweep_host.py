"""Threshold tuning without a GPU: the threshold grid and the logit cuts (eval/tune_threshold.py), the cuts
against the reference's own formulation (torch.sigmoid -> float16 -> `>=`), the counting of s2h_mask_sweep
(csrc/sweep_hist.h) compiled for the host and run in the kernel's decomposition (csrc/sweep_host_check.cpp, also
under the address and undefined-behaviour sanitizers, as a program), and SweepAccumulator against grid_search
over a synthetic dump."""
import json
import math
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import sweep_ref as R
from sam2_video.data import rle
from sam2_video.eval import tune_threshold as TT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sam2-video-training_amd", "csrc")
SHAPES = [(7, 9), (8, 8), (9, 7), (16, 4), (33, 65), (1, 1)]
DEFAULT = [0.2, 0.25, 0.3, 0.35, 0.4, 0.45, 0.5, 0.55, 0.6, 0.65, 0.7, 0.75, 0.8]


def test_threshold_grid_defaults():
    assert TT.threshold_grid() == DEFAULT and len(DEFAULT) == 13
    assert TT.threshold_grid(0.3, 0.5, 0.1) == [0.3, 0.4, 0.5]
    assert TT.threshold_grid(0.5, 0.5, 0.05) == [0.5]


@pytest.mark.parametrize("bad", [0.0, -0.1, 1.0001, 2.0, float("nan"), float("inf")])
def test_bad_thresholds_raise(bad):
    with pytest.raises(ValueError):
        TT.logit_cuts([0.5, bad])
    with pytest.raises(ValueError):
        TT.SweepAccumulator([bad], {"annotations": []}, 1000)


def test_accumulator_wants_ascending_thresholds():
    with pytest.raises(ValueError):
        TT.SweepAccumulator([0.5, 0.4], {"annotations": []}, 1000)
    with pytest.raises(ValueError):
        TT.SweepAccumulator([], {"annotations": []}, 1000)


def test_logit_cuts_are_the_smallest_float32_on_the_included_side():
    ts = DEFAULT + [0.5, 0.999, 0.001, 0.0004, 1.0]
    cuts = TT.logit_cuts(ts)
    assert cuts.dtype == np.float32 and cuts.shape == (len(ts),)
    assert cuts[DEFAULT.index(0.5)] == np.float32(-4.8828125e-4)
    for t, c in zip(ts, cuts):
        mid, inclusive = TT.threshold_mid(t)
        h = np.float16(t)
        lo = np.nextafter(h, np.float16(-1))
        assert lo < h and mid == (float(h) + float(lo)) / 2 and inclusive == (int(h.view(np.uint16)) % 2 == 0)
        below = np.nextafter(c, np.float32(-np.inf))
        p_in, p_out = float(R.sigmoid64(c)), float(R.sigmoid64(below))
        assert p_out < mid < p_in or (inclusive and p_out < mid == p_in), (t, c, p_out, mid, p_in)
        # and the float16 rounding of the exact sigmoid agrees: included at the cut, excluded one step below
        assert np.float16(p_in) >= h and np.float16(p_out) < h
    assert np.all(np.diff(TT.logit_cuts(DEFAULT)) > 0)
    # a threshold that rounds to float16 zero admits every probability
    assert TT.logit_cuts([1e-9])[0] == -np.inf


def _upsampled(seed, shape):
    g = torch.Generator().manual_seed(seed)
    low = 4 * torch.randn(13, 8, 8, generator=g)
    return torch.nn.functional.interpolate(low[None], size=shape, mode="bilinear", align_corners=False)[0].numpy()


def test_cuts_against_the_reference_formulation():
    """torch.sigmoid (fp32, CPU) -> float16 -> `>= thr` and `v >= cut(thr)` differ only on ambiguous pixels
    (|sigmoid64(v) - mid| <= 2^-22), and those are at most 1e-4 of the pixel-threshold pairs"""
    pairs = amb = diff = 0
    for seed in range(20):
        for shape in SHAPES:
            v = _upsampled(seed, shape)
            a = R.ambiguous(v, DEFAULT)
            d = R.reference_pixels(v, DEFAULT) != R.cut_pixels(v, DEFAULT)
            assert not (d & ~a).any(), (seed, shape, v[(d & ~a).any(axis=0)])
            pairs, amb, diff = pairs + a.size, amb + int(a.sum()), diff + int(d.sum())
    print(f"{pairs} pixel-threshold pairs, {amb} ambiguous, {diff} of them differ")
    assert amb <= 1e-4 * pairs


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def host_check(request, tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build csrc/sweep_host_check.cpp")
    exe = tmp_path_factory.mktemp("sweep_host") / f"sweep_host_check_{request.param}"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", *flags, "-I", CSRC,
                    os.path.join(CSRC, "sweep_host_check.cpp"), "-o", str(exe)], check=True)
    return str(exe)


def pack(m, dirty=False):
    """column-major bit packing of bool [H, W]; dirty: ones in the unused tail bits"""
    flat = np.asarray(m, bool).T.reshape(-1)
    nw = (flat.size + 63) // 64
    padded = np.full(nw * 64, bool(dirty))
    padded[:flat.size] = flat
    return np.packbits(padded.reshape(nw, 64), axis=1, bitorder="little").view("<u8").reshape(nw)


def run_cases(exe, tmp_path, cases):
    """cases: [(m fp32 [ncat, H, W], cuts fp32 [K], gt words uint64 [ncat, nw] or None)] -> [hist]"""
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        for m, cuts, gt in cases:
            ncat, H, W = m.shape
            f.write(np.asarray([ncat, H, W, len(cuts), int(gt is not None)], np.int32).tobytes())
            f.write(np.asarray(cuts, "<f4").tobytes())
            f.write(np.ascontiguousarray(m.transpose(0, 2, 1), "<f4").tobytes())  # column-major pixels
            if gt is not None:
                f.write(np.ascontiguousarray(gt, "<u8").tobytes())
    subprocess.run([exe, str(src), str(dst)], check=True, timeout=120)
    raw = np.frombuffer(dst.read_bytes(), np.int32)
    out, off = [], 0
    for m, cuts, _ in cases:
        n = m.shape[0] * 2 * (len(cuts) + 1)
        out.append(raw[off:off + n].reshape(m.shape[0], 2, len(cuts) + 1))
        off += n
    assert off == raw.size
    return out


def cuts_of(K, rng):
    if K == 13:
        return TT.logit_cuts(DEFAULT)
    c = np.sort(rng.normal(0, 3, K)).astype(np.float32)
    if K > 2:
        c[K // 2] = c[K // 2 - 1]  # equal neighbours: an empty bin
    return c


@pytest.mark.parametrize("shape", SHAPES + [(40, 60), (1, 1025)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_histogram_matches_numpy(host_check, tmp_path, shape):
    """(40 x 60 = 2400 and 1 x 1025 pixels: more than one workgroup of 1024, the last one partial)"""
    H, W = shape
    rng = np.random.default_rng(H * 131 + W)
    cases, want = [], []
    for K in (1, 13, 64):
        cuts = cuts_of(K, rng)
        m = rng.normal(0, 3, (5, H, W)).astype(np.float32)
        m[1] = cuts[0]                                  # exactly on a cut
        m[2] = np.nextafter(cuts[-1], np.float32(-np.inf))  # one step below the last one
        m[3].flat[::3] = np.nan
        m[3].flat[1::3] = -np.inf
        m[4].flat[::2] = np.inf
        gt = rng.random((5, H, W)) < 0.4
        for words in (None, np.stack([pack(g) for g in gt]), np.stack([pack(g, dirty=True) for g in gt])):
            cases.append((m, cuts, words))
            want.append(R.np_hist(m, [[c] for c in range(5)], cuts, None if words is None else gt))
    cases.append((np.zeros((0, H, W), np.float32), cuts_of(1, rng), None))  # no category at all
    want.append(np.zeros((0, 2, 2), np.int32))
    for (m, cuts, _), got, ref in zip(cases, run_cases(host_check, tmp_path, cases), want):
        assert np.array_equal(got, ref), (len(cuts), got, ref)
        assert np.all(got.sum(axis=(1, 2)) == H * W)


# ------------------------------------------------------------------------------------------- accumulator
MOD = 1000
FH, FW = 12, 10


def _rect(y0, y1, x0, x1):
    m = np.zeros((FH, FW), bool)
    m[y0:y1, x0:x1] = True
    return m


def _ann(image_id, cat, mask):
    return {"id": len(str(image_id)) * 1000 + cat, "image_id": image_id, "category_id": cat,
            "segmentation": rle.encode(mask), "iscrowd": 0}


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    """three dumped frames and one frame without objects (listed in meta.json, no .npz); objects 1 and 1001
    (category 1), 2 (category 2), 1000 (category 0) and 5 (category 5, never in the ground truth); category 7
    only in the ground truth; an annotation of category 8 with an empty mask (skipped, as neither predicted
    nor present)"""
    d = tmp_path_factory.mktemp("dump") / "probs"
    d.mkdir()
    obj_ids = np.asarray([1, 2, 1001, 1000, 5], np.int64)
    rng = np.random.default_rng(7)
    frames, anns = {}, []
    for image_id in (11, 12, 13):
        v = (3 * rng.normal(size=(len(obj_ids), FH, FW))).astype(np.float32)
        v[0, 2:9, 1:7] += 4
        v[1, 5:11, 4:9] += 4
        assert not R.ambiguous(v, DEFAULT).any()  # so `float16 probability >= thr` is `v >= cut` on every pixel
        frames[image_id] = v
        probs = R.sigmoid64(v).astype(np.float16)
        np.savez_compressed(d / f"{image_id}.npz", probs=probs, obj_ids=obj_ids, image_id=np.int64(image_id),
                            video_id="v0", order_in_video=np.int64(image_id - 10), height=np.int32(FH),
                            width=np.int32(FW))
        anns += [_ann(image_id, 1, _rect(2, 9, 1, 7)), _ann(image_id, 1, _rect(0, 3, 0, 3)),
                 _ann(image_id, 2, _rect(5, 11, 4, 9))]
    anns += [_ann(11, 7, _rect(0, 4, 6, 10)), _ann(12, 0, _rect(8, 12, 0, 5)), _ann(13, 8, np.zeros((FH, FW), bool)),
             _ann(14, 1, _rect(1, 5, 1, 5))]  # (image 14: ground truth but no objects, hence no dump)
    with open(d / "meta.json", "w") as f:
        json.dump({"mod": MOD, "image_ids": [11, 12, 13, 14], "dtype": "float16"}, f)
    return str(d), {"annotations": anns}, obj_ids, frames


def _accumulate(dump, thresholds, exclude_background):
    _, coco, obj_ids, frames = dump
    acc = TT.SweepAccumulator(thresholds, coco, MOD, exclude_background)
    cat_ids = list(dict.fromkeys(int(i) % MOD for i in obj_ids))
    cats = [[k for k, i in enumerate(obj_ids) if i % MOD == c] for c in cat_ids]
    from sam2_video.kernels.ops import pack_mask_bits
    for image_id, v in frames.items():
        words = acc.gt_bits(image_id, cat_ids, FH, FW)
        gt = np.stack([np.logical_or.reduce([rle.decode(a["segmentation"]).astype(bool)
                                             for a in coco["annotations"]
                                             if a["image_id"] == image_id and a["category_id"] == c] +
                                            [np.zeros((FH, FW), bool)]) for c in cat_ids])
        assert words.dtype == np.int64 and np.array_equal(words, pack_mask_bits(gt))
        assert np.array_equal(words.view("<u8"), np.stack([pack(g) for g in gt]))
        acc.add_frame(image_id, obj_ids, cat_ids, R.np_hist(v, cats, acc.cuts, gt))
    acc.add_frame(14, [], [], np.zeros((0, 2, len(thresholds) + 1), np.int32))  # no objects: nothing to add
    return acc


@pytest.mark.parametrize("exclude_background", [False, True], ids=["with_background", "exclude_background"])
def test_accumulator_equals_grid_search(dump, exclude_background):
    probs_dir, coco, _, _ = dump
    want = TT.grid_search(probs_dir, coco, exclude_background=exclude_background)
    acc = _accumulate(dump, TT.threshold_grid(), exclude_background)
    got = acc.result()
    assert got[0] == want[0] and abs(got[1] - want[1]) <= 1e-12
    assert [t for t, _ in got[2]] == [t for t, _ in want[2]] == DEFAULT
    for (t, a), (_, b) in zip(got[2], want[2]):
        assert abs(a - b) <= 1e-12, (t, a, b)
    # per image and threshold: categories 0 (image 12's ground truth, or predicted), 1, 2, 5 and image 11's 7
    n = 3 * 4 + 1 - (3 if exclude_background else 0)
    assert list(acc.count) == [n] * 13
    # the coco argument may be a path as well
    path = os.path.join(os.path.dirname(probs_dir), "coco.json")
    with open(path, "w") as f:
        json.dump(coco, f)
    assert TT.grid_search(probs_dir, path, exclude_background=exclude_background) == want
    with pytest.raises(ValueError):
        acc.add_frame(11, [1], [1], np.zeros((1, 2, 14), np.int32))  # a frame counts once


def test_background_changes_the_curve(dump):
    a = TT.grid_search(dump[0], dump[1], exclude_background=False)
    b = TT.grid_search(dump[0], dump[1], exclude_background=True)
    assert a[2] != b[2]


def test_gt_bits_refuses_another_size(dump):
    acc = TT.SweepAccumulator(DEFAULT, dump[1], MOD)
    with pytest.raises(ValueError):
        acc.gt_bits(11, [1, 2], FH + 1, FW)


def test_equal_maxima_go_to_the_threshold_closest_to_one_half(tmp_path):
    """one object whose probabilities are 0.9 inside its ground truth and 0.1 outside: every threshold of the
    grid gives Dice 1, and 0.5 wins; with the grid 0.2 .. 0.4 the closest one, 0.4"""
    gt = _rect(3, 8, 2, 7)
    v = np.where(gt, 2.2, -2.2).astype(np.float32)[None]
    d = tmp_path / "probs"
    d.mkdir()
    np.savez_compressed(d / "1.npz", probs=R.sigmoid64(v).astype(np.float16), obj_ids=np.asarray([3], np.int64),
                        height=np.int32(FH), width=np.int32(FW))
    TT.write_meta(str(d), MOD)
    coco = {"annotations": [_ann(1, 3, gt)]}
    for grid, best in (((0.2, 0.8, 0.05), 0.5), ((0.2, 0.4, 0.05), 0.4), ((0.6, 0.8, 0.1), 0.6)):
        ts = TT.threshold_grid(*grid)
        want = TT.grid_search(str(d), coco, *grid)
        # (Dice of a perfect 25-pixel mask: 50 / (50 + 1e-7) = 1 - 2e-9)
        assert want[0] == best and abs(want[1] - 1.0) <= 3e-9 and len({x for _, x in want[2]}) == 1
        acc = TT.SweepAccumulator(ts, coco, MOD)
        acc.add_frame(1, [3], [3], R.np_hist(v, [[0]], acc.cuts, gt[None]))
        assert acc.result() == want


def test_no_samples_is_an_error_and_the_payload_is_the_references(dump, tmp_path):
    with pytest.raises(RuntimeError):
        TT.SweepAccumulator(DEFAULT, {"annotations": []}, MOD).result()
    out = tmp_path / "best.json"
    TT.main(["--probs-dir", dump[0], "--coco-path", _write(tmp_path / "coco.json", dump[1]), "--output-json", str(out)])
    payload = json.load(open(out))
    assert list(payload) == ["best_threshold", "best_dice", "threshold_curve", "exclude_background", "range"]
    assert payload["range"] == {"min": 0.2, "max": 0.8, "step": 0.05} and payload["exclude_background"] is False
    want = TT.grid_search(dump[0], dump[1])
    assert payload["best_threshold"] == want[0] and [tuple(x) for x in payload["threshold_curve"]] == want[2]
    assert math.isfinite(payload["best_dice"])


def _write(path, obj):
    with open(path, "w") as f:
        json.dump(obj, f)
    return str(path)


def test_export_predict_from_a_dump(dump, tmp_path):
    """the host A/B path: per frame and category the `>=`-thresholded OR, its RLE, corners and the maximum
    float16 probability; category 0 dropped on request; indent=2 and the reference's default name"""
    from sam2_video.eval.export_predict_from_probs import export_predict
    from sam2_video.eval.utils import mask_to_bbox
    probs_dir, _, obj_ids, frames = dump
    path = export_predict(probs_dir, 0.35)
    assert path == os.path.join(os.path.dirname(probs_dir), "predict_t0.35.json")
    text = open(path).read()
    assert text.startswith("[\n  {\n    \"image_id\"")
    anns = json.loads(text)
    cut = TT.logit_cuts([0.35])[0]
    seen = set()
    for a in anns:
        v = frames[a["image_id"]]
        ks = [k for k, i in enumerate(obj_ids) if i % MOD == a["category_id"]]
        m = np.logical_or.reduce([v[k] >= cut for k in ks])
        assert a["segmentation"] == rle.encode(m) and a["bbox"] == mask_to_bbox(m) and a["iscrowd"] == 0
        assert a["score"] == float(np.float16(R.sigmoid64(max(v[k].max() for k in ks))))
        seen.add((a["image_id"], a["category_id"]))
    assert seen == {(i, c) for i in (11, 12, 13) for c in (1, 2, 0, 5)}
    no_bg = json.load(open(export_predict(probs_dir, 0.35, str(tmp_path / "p.json"), exclude_background=True)))
    assert {(a["image_id"], a["category_id"]) for a in no_bg} == {k for k in seen if k[1] != 0}
