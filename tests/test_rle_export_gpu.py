"""The fused mask export (s2h_mask_export) and the run-boundary extraction (s2h_rle_transitions) against a host
oracle built from the kernel they must agree with: ops.bilinear on the GPU -> .cpu() -> numpy `> 0`,
np.logical_or per category, rle.encode, numpy mask_to_bbox and sum.  Strings, areas, bounding boxes and the
set of empty categories are compared exactly; scores within 1e-5 of a float64 mean and bit-equal between runs."""
import numpy as np
import pytest
import torch

from sam2_video.data import rle

pytestmark = pytest.mark.gpu

SHAPES = [(7, 9), (8, 8), (9, 7), (16, 4), (33, 65), (1, 1)]
# object lists of the categories of the crafted call: zero objects, three objects out of index order, ...
CATS = [[2, 0], [], [12, 5, 7], [4], [3], [1, 6, 8, 9, 10, 11]]


def csr(cats, device="cuda"):
    off = np.cumsum([0] + [len(c) for c in cats]).astype(np.int32)
    obj = np.asarray([o for c in cats for o in c] + [0], np.int32)
    return torch.from_numpy(off).to(device), torch.from_numpy(obj).to(device)


def run_export(low, H, W, cats, non_overlap=False, capacity=None, bufs=None):
    """-> (hdr [ncat, 8], trans, scores) as numpy; bufs: (bits, scores, hdr, trans) device buffers to reuse"""
    from sam2_video.kernels import ops
    off, obj = csr(cats)
    if bufs is None:
        bits, sc = ops.mask_export(low, H, W, off, obj, len(cats), non_overlap)
        hdr, trans = ops.rle_transitions(bits, H, W, capacity=capacity)
    else:
        bits, sc = ops.mask_export(low, H, W, off, obj, len(cats), non_overlap, bits=bufs[0], scores=bufs[1])
        hdr, trans = ops.rle_transitions(bits, H, W, hdr=bufs[2], trans=bufs[3])
    return hdr.cpu().numpy(), trans.cpu().numpy(), sc.cpu().numpy(), bits


def oracle(low, H, W, cats, non_overlap=False):
    """-> (per category (counts string, area, bbox or None), float64 scores)"""
    from sam2_video.kernels import ops
    from sam2_video.predictor import SAM2VideoPredictor
    v = ops.bilinear(low, H, W)
    if non_overlap:
        v = SAM2VideoPredictor._apply_non_overlapping_constraints(v[:, None])[:, 0]
    v = v.cpu().numpy()
    out = []
    for objs in cats:
        m = np.logical_or.reduce([v[o] > 0 for o in objs], axis=0) if objs else np.zeros((H, W), bool)
        ys, xs = np.nonzero(m)
        box = None if ys.size == 0 else [int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())]
        out.append((rle.encode(m)["counts"], int(m.sum()), box, m))
    scores = (1.0 / (1.0 + np.exp(-v.astype(np.float64)))).reshape(v.shape[0], -1).mean(axis=1)
    return out, scores


def compare(got, want, H, W):
    hdr, trans, scores = got[:3]
    cats, ref_scores = want
    total, off = int(sum(h[0] for h in hdr)), 0
    for c, (counts, area, box, _) in enumerate(cats):
        n, o = int(hdr[c, 0]), int(hdr[c, 1])
        assert o == off and hdr[c, 7] == total
        off += n
        assert int(hdr[c, 2]) == area, f"area of category {c}"
        assert (int(hdr[c, 2]) == 0) == (box is None)
        assert rle.from_transitions(trans[o:o + n], H, W)["counts"] == counts, f"runs of category {c}"
        if box is not None:
            assert [int(x) for x in hdr[c, 3:7]] == box, f"bbox of category {c}"
    print("max score error", np.abs(scores - ref_scores).max() if len(scores) else 0.0)
    assert np.abs(scores - ref_scores).max(initial=0.0) <= 1e-5


def last_pixel_plane(H, W, hi=8, wi=8):
    """a low-res plane whose upsampling is positive only where the last pixel's own tap weighs most"""
    def weights(n_out, n_in):  # weight each output gives to the last output's upper tap
        s = np.maximum(n_in / n_out * (np.arange(n_out) + 0.5) - 0.5, 0.0)
        i0 = np.minimum(s.astype(np.int64), n_in - 1)
        i1 = i0 + (i0 < n_in - 1)
        l1 = s - i0
        t = i1[-1]
        return t, (i0 == t) * (1 - l1) + (i1 == t) * l1
    ty, wy = weights(H, hi)
    tx, wx = weights(W, wi)
    prod = np.outer(wy, wx)
    top = prod[-1, -1]
    assert top == prod.max()
    rest = prod[prod < top]
    second = rest.max() if rest.size else 0.0
    p = -np.ones((hi, wi), np.float32)
    p[ty, tx] = -1.0 + 2.0 / (top + second)
    return p, prod == top


def crafted(H, W):
    g = torch.Generator().manual_seed(H * 100 + W)
    low = torch.randn(13, 8, 8, generator=g)
    low[0] = -1.0
    low[1] = 1.0
    low[2] = 0.0
    low[2, :, 4:] = -0.0
    lp, where = last_pixel_plane(H, W)
    low[3] = torch.from_numpy(lp)
    yy, xx = np.mgrid[:8, :8]
    low[4] = torch.from_numpy(np.where((yy + xx) % 2 == 0, 1.0, -1.0).astype(np.float32))
    return low.cuda().contiguous(), where


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_crafted_planes_match_the_host_oracle(shape):
    H, W = shape
    low, where = crafted(H, W)
    want = oracle(low, H, W, CATS)
    # the crafted objects are what they claim
    assert want[0][0][1] == 0 and want[0][1][1] == 0 and want[0][5][1] == H * W  # 0.0 / -0.0 / negative: empty
    assert np.array_equal(want[0][4][3], where) and where[-1, -1]
    # one pixel, but at 33 x 65: there the source coordinate clamps to the last low-res row / column for the
    # last 2 rows and 4 columns, which all read the same value (a 2 x 4 corner block ending in the last pixel)
    assert where.sum() == (8 if shape == (33, 65) else 1)
    if shape == (8, 8):
        assert want[0][3][1] == 32 and want[0][3][0] == rle.encode((np.add(*np.mgrid[:8, :8]) % 2) == 0)["counts"]
    got = run_export(low, H, W, CATS)
    compare(got, want, H, W)
    # capacity overflow: the header reports the total, the buffer holds the first `cap` positions, nothing
    # behind them is touched, and the re-run with the reported capacity is complete
    total = int(got[0][0, 7])
    cap = total // 2
    from sam2_video.kernels import ops
    guard = torch.full((cap + 8,), -7, device="cuda", dtype=torch.int32)
    hdr2, _ = ops.rle_transitions(got[3], H, W, trans=guard[:cap])
    assert np.array_equal(hdr2.cpu().numpy(), got[0])
    assert np.array_equal(guard.cpu().numpy(), np.concatenate([got[1][:cap], np.full(8, -7, np.int32)]))
    hdr3, trans3 = ops.rle_transitions(got[3], H, W, capacity=int(hdr2[0, 7]))
    compare((hdr3.cpu().numpy(), trans3.cpu().numpy(), got[2]), want, H, W)


@pytest.mark.parametrize("non_overlap", [False, True], ids=["overlap", "non_overlap"])
def test_thirteen_objects_in_four_categories(non_overlap):
    """the evaluation's own layout: N = 13 in exactly 4 categories, none empty, members out of index order"""
    cats = [[12, 0, 5], [1, 2, 3, 4], [11, 6], [7, 10, 9, 8]]
    assert sorted(o for c in cats for o in c) == list(range(13))
    for H, W in ((33, 65), (9, 7)):
        low, _ = crafted(H, W)
        compare(run_export(low, H, W, cats, non_overlap), oracle(low, H, W, cats, non_overlap), H, W)


def test_single_object():
    low, _ = crafted(9, 7)
    for i in (0, 1, 4, 6):
        one = low[i:i + 1].contiguous()
        compare(run_export(one, 9, 7, [[0]]), oracle(one, 9, 7, [[0]]), 9, 7)


def test_two_frames_through_the_same_buffers():
    """a stale word, header field or position of the first frame would show in the second"""
    from sam2_video.kernels import ops
    H, W = 33, 65
    a, _ = crafted(H, W)
    b = (-a).flip(0).contiguous()
    b[4] = -1.0  # far fewer runs than the checkerboard left behind
    ncat, nw = len(CATS), ops.rle_words(H, W)
    bufs = (torch.empty(ncat, nw, device="cuda", dtype=torch.int64), torch.empty(13, device="cuda"),
            torch.empty(ncat, 8, device="cuda", dtype=torch.int32),
            torch.empty(ncat * H * W, device="cuda", dtype=torch.int32))
    for x in (a, b, a):
        compare(run_export(x, H, W, CATS, bufs=bufs), oracle(x, H, W, CATS), H, W)


@pytest.fixture(scope="module")
def large():
    """64^2 -> 517 x 1031: 8329 words = 33 scan blocks per category, odd sizes; smooth logits and one object
    of 0.59-density noise"""
    g = torch.Generator().manual_seed(11)
    smooth = torch.nn.functional.avg_pool2d(torch.randn(4, 1, 64, 64, generator=g), 5, stride=1, padding=2)[:, 0]
    noise = torch.where(torch.rand(1, 64, 64, generator=g) < 0.59, 1.0, -1.0)
    low = torch.cat([smooth, noise]).cuda().contiguous()
    cats = [[4, 1], [0, 2, 3]]
    return low, cats, oracle(low, 517, 1031, cats)


def test_large_odd_case(large):
    low, cats, want = large
    got = run_export(low, 517, 1031, cats)
    compare(got, want, 517, 1031)
    assert got[0][0, 7] > 4 * 256  # many transitions per scan block


def test_scores_are_bit_reproducible(large):
    low, cats, _ = large
    a = run_export(low, 517, 1031, cats)[2]
    b = run_export(low, 517, 1031, cats)[2]
    assert np.array_equal(a.view(np.int32), b.view(np.int32))


def test_non_overlap_first_index_wins_ties():
    H, W = 33, 65
    g = torch.Generator().manual_seed(3)
    low = torch.randn(6, 8, 8, generator=g)
    low[5] = low[2]  # identical objects: the lower index keeps the pixels, object 5 keeps none
    low = low.cuda().contiguous()
    cats = [[0, 1], [2], [5], [3, 4]]
    want = oracle(low, H, W, cats, non_overlap=True)
    assert want[0][2][1] == 0 and want[0][1][1] > 0
    compare(run_export(low, H, W, cats, non_overlap=True), want, H, W)
    # and the flag really changes the result
    assert oracle(low, H, W, cats)[0][2][1] > 0


def test_export_in_a_hip_graph():
    """both calls on one stream, no parallel branches; the scratch comes from the graph's pool.  Replayed with
    two contents of the static input, each equal to the eager result."""
    from sam2_video.kernels import ops
    H, W = 33, 65
    a, _ = crafted(H, W)
    b = (-a).flip(0).contiguous()
    off, obj = csr(CATS)
    static_in = a.clone()
    run_export(static_in, H, W, CATS)  # eager warm-up
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        bits, sc = ops.mask_export(static_in, H, W, off, obj, len(CATS), False)
        hdr, trans = ops.rle_transitions(bits, H, W)
    for x in (b, a):
        static_in.copy_(x)
        g.replay()
        torch.cuda.synchronize()
        eager = run_export(x, H, W, CATS)
        assert np.array_equal(hdr.cpu().numpy(), eager[0])
        n = int(eager[0][0, 7])
        assert np.array_equal(trans.cpu().numpy()[:n], eager[1][:n])
        assert np.array_equal(sc.cpu().numpy().view(np.int32), eager[2].view(np.int32))


def test_merged_frame_reruns_past_its_capacity(large):
    """MergedFrame.result() with a buffer that is too small reads the needed capacity from the header and
    extracts again: the same result as with room to spare, and as the host oracle"""
    from sam2_video.predictor import MergedFrame
    low, cats, want = large
    off, obj = csr(cats)
    args = (low, 517, 1031, [7, 8, 9, 10, 11], ["a", "b"], off, obj)
    roomy, tight = MergedFrame(*args, capacity=None), MergedFrame(*args, capacity=5)
    a, b = roomy.result(), tight.result()
    assert a == b and list(a["scores"]) == [7, 8, 9, 10, 11]
    total = tight.runs_total  # the header's total
    assert roomy.runs_total == total and tight.staging is None and roomy.staging is None
    assert total > 5 and tight.bytes_copied == (2 * 8 + 5 + 5 + total) * 4  # the overflow really happened
    for c, name in enumerate(["a", "b"]):
        assert a["categories"][name]["segmentation"] == {"size": [517, 1031], "counts": want[0][c][0]}
        assert a["categories"][name]["area"] == want[0][c][1]
        assert a["categories"][name]["bbox"] == [float(v) for v in want[0][c][2]]


def test_sizes_outside_the_limits_are_refused():
    from sam2_video.kernels import _lib, ops
    low = torch.zeros(1, 8, 8, device="cuda")
    off, obj = csr([[0]])
    bits = torch.zeros(1, 1, device="cuda", dtype=torch.int64)
    with pytest.raises(_lib.HipKernelError):  # H W > 2^24
        _lib.call("s2h_mask_export", 1, 8, 8, 4097, 4096, low.data_ptr(), 1, off.data_ptr(), obj.data_ptr(), 0,
                  bits.data_ptr(), low.data_ptr(), low.data_ptr(), None)
    with pytest.raises(_lib.HipKernelError):  # Ncat H W >= 2^31 - 256
        _lib.call("s2h_rle_transitions", 1024, 2048, 2048, bits.data_ptr(), 0, bits.data_ptr(), None,
                  bits.data_ptr(), None)
    assert ops.rle_words(1, 1) == 1 and ops.rle_words(8, 8) == 1 and ops.rle_words(5, 13) == 2
