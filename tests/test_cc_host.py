"""Connected components / hole filling without a GPU: the union-find header the kernels are built from
(csrc/cc_uf.h), compiled for the host and run sequentially (csrc/cc_host_check.cpp), against
scipy.ndimage.label on the pattern list of cc_patterns.py; the predictor's CPU path and the binding."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import cc_patterns as cp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sam2-video-training_amd", "csrc")


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build csrc/cc_host_check.cpp")
    exe = tmp_path_factory.mktemp("cc_host") / "cc_host_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC,
                    os.path.join(CSRC, "cc_host_check.cpp"), "-o", str(exe)], check=True)
    return str(exe)


def _run(exe, tmp_path, cases):
    """cases: [(mode, arg, scores [N, H, W] fp32)] -> the raw output bytes"""
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        for mode, arg, s in cases:
            N, H, W = s.shape
            f.write(np.asarray([mode, N, H, W, arg], np.int32).tobytes())
            f.write(np.ascontiguousarray(s, np.float32).tobytes())
    subprocess.run([exe, str(src), str(dst)], check=True, timeout=120)
    return dst.read_bytes()


@pytest.mark.parametrize("shape", cp.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_union_find_header_matches_scipy(host_check, tmp_path, shape):
    H, W = shape
    names, scores, ref = cp.shape_case(H, W)
    P = len(names)
    # batches of 1, 3 and 13 different images, both polarities, in one run of the program
    cases, want = [], []
    for N in cp.BATCHES:
        for idx in cp.chunks(P, N):
            for positive in (True, False):
                cases.append((0, int(positive), scores[idx]))
                want.append((idx, positive))
    raw = np.frombuffer(_run(host_check, tmp_path, cases), np.int32)
    assert raw.size == sum(2 * len(idx) * H * W for idx, _ in want)
    off = 0
    for idx, positive in want:
        n = len(idx) * H * W
        labels = raw[off:off + n].reshape(len(idx), H, W)
        areas = raw[off + n:off + 2 * n].reshape(len(idx), H, W)
        off += 2 * n
        rl, ra = ref[positive]
        for j, k in enumerate(idx):
            assert np.array_equal(labels[j], rl[k]), f"labels of {names[k]} positive={positive} N={len(idx)}"
            assert np.array_equal(areas[j], ra[k]), f"areas of {names[k]} positive={positive} N={len(idx)}"


def test_reference_patterns_are_what_they_claim():
    """the checkerboard is one component under 8-connectivity, the serpentine one chain of about half the
    pixels, the rings nested and separate, the noise levels span many-small to one component"""
    names, _, ref = cp.shape_case(128, 128)
    lab, area = ref[True]
    comps = {k: int(np.count_nonzero(np.unique(lab[i]))) for i, k in enumerate(names)}
    assert comps["checkerboard"] == 1 and comps["all_foreground"] == 1 and comps["all_background"] == 0
    assert comps["serpentine"] == 1 and area[names.index("serpentine")].max() == 64 * 128 + 64
    assert comps["spiral"] == 1 and comps["main_diagonal"] == 1 and comps["anti_diagonal"] == 1
    assert comps["rings"] == len(range(0, 64, 3))
    assert comps["noise_p0.3_s0"] > 500 and comps["noise_p0.9_s0"] == 1
    assert area[names.index("noise_p0.59_s0")].max() > 128 * 128 // 2


@pytest.mark.parametrize("max_area", cp.MAX_AREAS)
def test_host_fill_holes_matches_predictor_host_path(host_check, tmp_path, max_area):
    inputs = cp.fill_inputs()
    names = [k for k in inputs if k != "smooth256"]  # (the GPU test covers it; the scipy side is the slow one)
    cases = [(1, max_area, inputs[k][:, 0].numpy()) for k in names]
    raw = np.frombuffer(_run(host_check, tmp_path, cases), np.float32)
    off = 0
    for k in names:
        want = cp.fill_reference(k, max_area)
        got = torch.from_numpy(raw[off:off + want.numel()].copy()).view_as(want)
        off += want.numel()
        # bit for bit (view as int32: -0.0 stays -0.0)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), k
    assert off == raw.size


def test_ordering_case_keeps_the_ring():
    out = cp.fill_reference("ordering", 8)
    assert out[0, 0, 3, 3] == np.float32(0.1)
    ring = out[0, 0, 2:5, 2:5].clone()
    ring[1, 1] = 1.0
    assert torch.all(ring == 1.0) and torch.all(out[0, 0, :2] == -2.0)


def test_cpu_tensors_still_take_scipy(monkeypatch):
    from sam2_video import predictor
    from sam2_video.kernels import ops

    def boom(*a, **k):
        raise AssertionError("a CPU tensor must not reach the HIP kernels")

    monkeypatch.setattr(ops, "fill_holes", boom)
    calls = []
    real = predictor._connected_components
    monkeypatch.setattr(predictor, "_connected_components", lambda b: (calls.append(1), real(b))[1])
    x = cp.ordering_case()
    out = predictor.fill_holes_in_mask_scores(x.clone(), 8)
    assert len(calls) == 2 and not out.is_cuda and out[0, 0, 3, 3] == np.float32(0.1)
    with pytest.raises(RuntimeError):
        predictor.get_connected_components(torch.zeros(1, 1, 4, 4, dtype=torch.bool))


def test_binding_declares_the_new_entry_points():
    from sam2_video.kernels import _lib, ops
    from sam2_video.predictor import SAM2VideoPredictor
    import inspect
    assert len(_lib.SIGNATURES["s2h_cc_label"]) == 8 and len(_lib.SIGNATURES["s2h_fill_holes"]) == 8
    assert callable(ops.cc_label) and callable(ops.fill_holes)
    assert inspect.signature(SAM2VideoPredictor.__init__).parameters["postprocess_on_device"].default is True
