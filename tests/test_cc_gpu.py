"""The connected-components and hole-filling kernels (csrc/cc.hip) against scipy, exactly: labels made
canonical (1 + the smallest row-major index of the component), areas from bincount; the device hole
filling against the predictor's host path; capture in a HIP graph; upstream's get_connected_components
contract.  Inputs and references: cc_patterns.py (computed once per shape, shared, read-only)."""
import numpy as np
import pytest
import torch

import cc_patterns as cp

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("positive", [True, False], ids=["pos", "neg"])
@pytest.mark.parametrize("N", cp.BATCHES)
@pytest.mark.parametrize("shape", cp.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_cc_label_equals_scipy(shape, N, positive):
    from sam2_video.kernels import ops
    H, W = shape
    names, scores, ref = cp.shape_case(H, W)
    rl, ra = ref[positive]
    dev_scores = torch.from_numpy(scores.copy()).cuda()
    for idx in cp.chunks(len(names), N):  # N different images per launch: a label leaking between slots shows
        labels, areas = ops.cc_label(dev_scores[idx].contiguous(), positive=positive)
        assert labels.dtype == torch.int32 and areas.dtype == torch.int32 and labels.shape == (N, H, W)
        labels, areas = labels.cpu(), areas.cpu()
        for j, k in enumerate(idx):
            assert torch.equal(labels[j], torch.tensor(rl[k])), f"labels: {names[k]} (slot {j} of {N})"
            assert torch.equal(areas[j], torch.tensor(ra[k])), f"areas: {names[k]} (slot {j} of {N})"


def test_cc_label_beyond_the_product_sizes():
    """517 x 1031 (odd: a row is 16 waves + 7 pixels): the serpentine is one chain of 267,287 pixels through
    some 2,080 workgroups, the 0.59 noise percolates; both polarities, a batch of two different images"""
    from sam2_video.kernels import ops
    H, W = 517, 1031
    pats = cp.patterns(H, W)
    scores = np.stack([cp.scores_of(pats[k]) for k in ("serpentine", "noise_p0.59_s1")])
    dev_scores = torch.from_numpy(scores).cuda()
    for positive in (True, False):
        labels, areas = ops.cc_label(dev_scores, positive=positive)
        for j in range(2):
            rl, ra = cp.reference(scores[j] > 0 if positive else scores[j] <= 0)
            assert torch.equal(labels[j].cpu(), torch.tensor(rl)) and torch.equal(areas[j].cpu(), torch.tensor(ra))


@pytest.mark.parametrize("max_area", cp.MAX_AREAS)
@pytest.mark.parametrize("name", list(cp.fill_inputs()))
def test_fill_holes_equals_host_path(name, max_area):
    from sam2_video.kernels import ops
    from sam2_video.predictor import fill_holes_in_mask_scores
    x = cp.fill_inputs()[name]
    want = cp.fill_reference(name, max_area)
    got = fill_holes_in_mask_scores(x.cuda(), max_area)  # [N, 1, H, W] through the public dispatch
    assert got.is_cuda and got.shape == x.shape and got.dtype == torch.float32
    assert torch.equal(got.cpu(), want), f"{(got.cpu() != want).sum().item()} of {want.numel()} elements differ"
    # untouched elements are copies bit for bit (-0.0 stays -0.0), the written ones exactly +-0.1f
    assert torch.equal(got.cpu().view(torch.int32), want.view(torch.int32))
    got3 = ops.fill_holes(x[:, 0].contiguous().cuda(), max_area)  # [N, H, W]
    assert torch.equal(got3.cpu(), want[:, 0])


def test_fill_holes_ordering_case():
    """the second pass sees the first one's result: the filled centre makes the ring 9 pixels > 8"""
    from sam2_video.kernels import ops
    out = ops.fill_holes(cp.ordering_case().cuda(), 8).cpu()
    expect = cp.ordering_case()
    expect[0, 0, 3, 3] = 0.1
    assert torch.equal(out, expect)
    # with the centre already positive the 3 x 3 block has area 9 and stays at max_area 8, goes at 9
    blk = cp.ordering_case()
    blk[0, 0, 3, 3] = 1.0
    assert torch.equal(ops.fill_holes(blk.cuda(), 8).cpu(), blk)
    gone = blk.clone()
    gone[0, 0, 2:5, 2:5] = -0.1
    assert torch.equal(ops.fill_holes(blk.cuda(), 9).cpu(), gone)


def test_fill_holes_in_a_hip_graph():
    """one stream, no parallel branches; the scratch comes from the graph's pool.  Two contents of the
    static input, each replay equal to the host path (which cannot be captured: it synchronises)."""
    from sam2_video.kernels import ops
    a, b = cp.fill_inputs()["smooth64"], cp.fill_inputs()["smooth64"].flip(0).neg().contiguous()
    static_in = a.cuda()
    ops.fill_holes(static_in, 8)  # eager warm-up
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        static_out = ops.fill_holes(static_in, 8)
    from sam2_video.predictor import fill_holes_in_mask_scores
    for x in (b, a):
        static_in.copy_(x)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(static_out.cpu(), fill_holes_in_mask_scores(x.clone(), 8))


def test_get_connected_components_upstream_contract():
    from sam2_video.predictor import get_connected_components
    H, W = 37, 53
    names, scores, ref = cp.shape_case(H, W)
    idx = [names.index(k) for k in ("rings", "noise_p0.3_s0", "all_background")]
    mask = torch.from_numpy(scores[idx] > 0)[:, None]  # [3, 1, H, W] bool
    for m in (mask.cuda(), mask.to(torch.uint8).cuda()):
        labels, counts = get_connected_components(m)
        assert labels.shape == counts.shape == (3, 1, H, W)
        assert labels.dtype == torch.int32 and counts.dtype == torch.int32 and labels.is_cuda
        assert torch.equal(labels[:, 0].cpu(), torch.tensor(ref[True][0][idx]))
        assert torch.equal(counts[:, 0].cpu(), torch.tensor(ref[True][1][idx]))
        bg = ~mask.cuda()
        assert (labels[bg] == 0).all() and (counts[bg] == 0).all() and (labels[~bg] > 0).all()
    with pytest.raises(AssertionError):
        get_connected_components(torch.zeros(H, W, dtype=torch.bool, device="cuda"))


def test_cc_label_rejects_sizes_outside_the_kernels_range():
    from sam2_video.kernels import _lib
    s = torch.zeros(4, device="cuda")
    lab = torch.zeros(4, device="cuda", dtype=torch.int32)
    with pytest.raises(_lib.HipKernelError):  # H * W > 2^24: refused before any launch
        _lib.call("s2h_cc_label", 1, 4097, 4096, s.data_ptr(), 1, lab.data_ptr(), lab.data_ptr(), None)
    with pytest.raises(_lib.HipKernelError):  # N * H * W past the int range the kernels index with
        _lib.call("s2h_cc_label", 1024, 2048, 2048, s.data_ptr(), 1, lab.data_ptr(), lab.data_ptr(), None)
    with pytest.raises(_lib.HipKernelError):  # in place
        _lib.call("s2h_fill_holes", 1, 2, 2, s.data_ptr(), 8, s.data_ptr(), lab.data_ptr(), None)
