"""The RLE export without a GPU: the host half of the codec (data/rle.py counts_from_transitions /
from_transitions) against rle.encode and against pycocotools' own strings (tests/golden), and the word-level
logic of the run-boundary kernels (csrc/rle_scan.h), compiled for the host and run sequentially in the
kernels' block decomposition (csrc/rle_host_check.cpp), against numpy."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from sam2_video.data import rle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sam2-video-training_amd", "csrc")
GOLD = os.path.join(ROOT, "tests", "golden", "rle_endovis18_sample.json")
SHAPES = [(1, 1), (1, 64), (64, 1), (7, 9), (5, 13), (63, 65)]
HDR = 8


def masks_of(h, w):
    """name -> bool [h, w]"""
    rng = np.random.default_rng(h * 131 + w)
    yy, xx = np.mgrid[:h, :w]
    m = {"zero": np.zeros((h, w), bool), "one": np.ones((h, w), bool),
         "first": np.zeros((h, w), bool), "last": np.zeros((h, w), bool),
         "checker": (yy + xx) % 2 == 1, "checker_first_set": (yy + xx) % 2 == 0,
         # vertical against horizontal stripes: on a non-square shape a row-major mix-up changes the runs
         "vstripes": np.broadcast_to(xx % 2 == 0, (h, w)).copy(), "hstripes": np.broadcast_to(yy % 2 == 0, (h, w)).copy()}
    m["first"][0, 0] = True
    m["last"][-1, -1] = True
    for p in (0.01, 0.5, 0.99):
        m[f"random_{p}"] = rng.random((h, w)) < p
    return m


def transitions(m):
    """numpy run boundaries of a mask: positions of the column-major flattening that differ from the pixel
    before them (the pixel before the first one counts as 0)"""
    flat = np.asarray(m, bool).T.reshape(-1).astype(np.int8)
    return np.flatnonzero(np.diff(np.concatenate([[0], flat])))


def pack(m, dirty=False):
    """column-major bit packing, bit j % 64 of word j // 64 = pixel j; dirty: ones in the unused tail bits"""
    flat = np.asarray(m, bool).T.reshape(-1)
    nw = (flat.size + 63) // 64
    padded = np.full(nw * 64, bool(dirty))
    padded[:flat.size] = flat
    return np.packbits(padded.reshape(nw, 64), axis=1, bitorder="little").view("<u8").reshape(nw)


def bbox_area(m):
    ys, xs = np.nonzero(m)
    if ys.size == 0:
        return [0, m.shape[1], m.shape[0], -1, -1]
    return [int(ys.size), int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_from_transitions_equals_encode(shape):
    h, w = shape
    for name, m in masks_of(h, w).items():
        t = transitions(m)
        got = rle.from_transitions(t, h, w)
        want = rle.encode(m)
        assert got == want, name
        assert np.array_equal(rle.decode(got), m.astype(np.uint8)), name
        cnts = rle.counts_from_transitions(t, h * w)
        assert sum(cnts) == h * w and (cnts[0] == 0) == bool(m[0, 0]), name
    if h != w and h > 1 and w > 1:
        ms = masks_of(h, w)
        assert rle.from_transitions(transitions(ms["vstripes"]), h, w) != \
            rle.from_transitions(transitions(ms["hstripes"].T), w, h)


def test_first_count_is_zero_when_the_first_pixel_is_set():
    assert rle.counts_from_transitions([0, 3], 6) == [0, 3, 3]
    assert rle.counts_from_transitions([], 6) == [6]
    assert rle.counts_from_transitions([0], 6) == [0, 6]
    assert rle.counts_from_transitions([5], 6) == [5, 1]


def test_pycocotools_strings_are_reproduced():
    gold = json.load(open(GOLD))
    n = 0
    for group in gold.values():
        for ann in group:
            seg = ann["segmentation"]
            h, w = seg["size"]
            m = rle.decode(seg)
            assert rle.from_transitions(transitions(m), h, w)["counts"] == seg["counts"]
            n += 1
    assert n > 0


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build csrc/rle_host_check.cpp")
    exe = tmp_path_factory.mktemp("rle_host") / "rle_host_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC,
                    os.path.join(CSRC, "rle_host_check.cpp"), "-o", str(exe)], check=True)
    return str(exe)


def run_cases(exe, tmp_path, cases):
    """cases: [(h, w, capacity, words uint64 [ncat, nw])] -> [(hdr int32 [ncat, 8], trans int32)]"""
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        for h, w, cap, words in cases:
            f.write(np.asarray([words.shape[0], h, w, cap], np.int32).tobytes())
            f.write(np.ascontiguousarray(words, "<u8").tobytes())
    subprocess.run([exe, str(src), str(dst)], check=True, timeout=120)
    raw = np.frombuffer(dst.read_bytes(), np.int32)
    out, off = [], 0
    for h, w, cap, words in cases:
        ncat = words.shape[0]
        hdr = raw[off:off + ncat * HDR].reshape(ncat, HDR)
        off += ncat * HDR
        n = min(int(hdr[0, 7]), cap) if ncat else 0
        out.append((hdr, raw[off:off + n]))
        off += n
    assert off == raw.size
    return out


def check(hdr, trans, masks, cap):
    """header and positions of one case against numpy"""
    want = [transitions(m) for m in masks]
    total = sum(t.size for t in want)
    allt = np.concatenate(want) if want else np.zeros(0, np.int64)
    off = 0
    for c, m in enumerate(masks):
        assert hdr[c, 0] == want[c].size and hdr[c, 1] == off and hdr[c, 7] == total
        assert list(hdr[c, 2:7]) == bbox_area(m), (c, list(hdr[c]), bbox_area(m))
        off += want[c].size
    assert np.array_equal(trans, allt[:cap])


@pytest.mark.parametrize("shape", SHAPES + [(9, 7), (1, 63), (13, 5), (127, 1)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_word_logic_matches_numpy(host_check, tmp_path, shape):
    h, w = shape  # (H W of 63, 64, 65 and 127 are among the shapes)
    ms = list(masks_of(h, w).values())
    cases, masks = [], []
    for dirty in (False, True):
        cases.append((h, w, len(ms) * h * w, np.stack([pack(m, dirty) for m in ms])))  # all as categories of one call
        masks.append(ms)
        for m in ms:  # and one by one
            cases.append((h, w, h * w, pack(m, dirty)[None]))
            masks.append([m])
    cases.append((h, w, 0, np.zeros((0, (h * w + 63) // 64), "<u8")))  # no category at all
    masks.append([])
    outs = run_cases(host_check, tmp_path, cases)
    for (_, _, cap, _), mm, (hdr, trans) in zip(cases, masks, outs):
        check(hdr, trans, mm, cap)


def test_runs_across_word_and_block_boundaries(host_check, tmp_path):
    """256 words = 16384 pixels per block: 130 x 257 = 33410 pixels are three blocks per category; runs that
    start in one word / block and end in the next, one pixel each side of the boundaries, and a run that
    covers a whole block"""
    h, w = 130, 257
    n = h * w
    flat = np.zeros((4, n), bool)
    flat[0, 60:70] = True          # crosses the first word boundary
    flat[0, 16380:16390] = True    # crosses the first block boundary
    flat[0, 127] = True            # last bit of a word
    flat[0, 128] = False
    flat[0, 192] = True            # first bit of a word
    flat[1, 16383] = True          # last pixel of block 0 alone
    flat[1, 16384 * 2] = True      # first pixel of block 2 alone
    flat[2, 100:16384 * 2 + 5] = True  # covers block 1 entirely
    flat[3, :] = True
    flat[3, 16384] = False
    masks = [f.reshape(w, h).T for f in flat]
    rng = np.random.default_rng(5)
    masks.append(rng.random((h, w)) < 0.5)
    words = np.stack([pack(m, True) for m in masks])
    total = sum(transitions(m).size for m in masks)
    outs = run_cases(host_check, tmp_path, [(h, w, total, words), (h, w, 7, words), (h, w, 0, words)])
    for cap, (hdr, trans) in zip((total, 7, 0), outs):
        check(hdr, trans, masks, cap)  # (capacity 7 and 0: the overflow report, nothing past the end)
        assert hdr[0, 7] == total


def test_binding_declares_the_export():
    import inspect
    from sam2_video.kernels import _lib, ops
    from sam2_video.predictor import MergedFrame, SAM2VideoPredictor
    assert len(_lib.SIGNATURES["s2h_mask_export"]) == 14 and len(_lib.SIGNATURES["s2h_rle_transitions"]) == 9
    assert callable(ops.mask_export) and callable(ops.rle_transitions) and ops.RLE_HDR == HDR
    assert "obj_to_cat" in inspect.signature(SAM2VideoPredictor.propagate_in_video_export).parameters
    assert callable(MergedFrame.result)
