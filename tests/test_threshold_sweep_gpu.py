"""The threshold sweep (s2h_mask_sweep) and the export at a cut (s2h_mask_export_cut) against a host oracle built
from the kernel they must agree with: ops.bilinear on the GPU -> .cpu() -> numpy `>=` (tests/sweep_ref.py), with
the shapes and category lists of tests/test_rle_export_gpu.py.  Histograms, bits and maxima are compared
exactly; the reference's formulation (torch.sigmoid -> float16 -> `>= thr`) on seeds without ambiguous pixels."""
import numpy as np
import pytest
import torch

import sweep_ref as R
from sam2_video.data import rle
from sam2_video.eval import tune_threshold as TT

pytestmark = pytest.mark.gpu

SHAPES = [(7, 9), (8, 8), (9, 7), (16, 4), (33, 65), (1, 1)]
CATS = [[2, 0], [], [12, 5, 7], [4], [3], [1, 6, 8, 9, 10, 11]]
DEFAULT = TT.threshold_grid()


def csr(cats, device="cuda"):
    off = np.cumsum([0] + [len(c) for c in cats]).astype(np.int32)
    obj = np.asarray([o for c in cats for o in c] + [0], np.int32)
    return torch.from_numpy(off).to(device), torch.from_numpy(obj).to(device)


def video_res(low, H, W, non_overlap=False):
    """the final values [N, H, W] as numpy: ops.bilinear (+ upstream's non-overlap clamp)"""
    from sam2_video.kernels import ops
    from sam2_video.predictor import SAM2VideoPredictor
    v = ops.bilinear(low, H, W)
    if non_overlap:
        v = SAM2VideoPredictor._apply_non_overlapping_constraints(v[:, None])[:, 0]
    return v.cpu().numpy()


def sweep(low, H, W, cats, cuts, gt_words=None, non_overlap=False, hist=None):
    from sam2_video.kernels import ops
    off, obj = csr(cats)
    gt = None if gt_words is None else torch.from_numpy(np.ascontiguousarray(gt_words)).cuda()
    out = ops.mask_sweep(low, H, W, off, obj, len(cats), torch.from_numpy(np.asarray(cuts, np.float32)).cuda(),
                         gt, non_overlap, hist=hist)
    return out.cpu().numpy()


def cuts_of(K, seed=0):
    if K == 13:
        return TT.logit_cuts(DEFAULT)
    c = np.sort(np.random.default_rng(seed + K).normal(0, 1.5, K)).astype(np.float32)
    if K > 2:
        c[K // 2] = c[K // 2 - 1]  # repeated cuts: an empty bin
    return c


def planes(H, W, seed=None):
    g = torch.Generator().manual_seed(H * 100 + W if seed is None else seed)
    return torch.randn(13, 8, 8, generator=g).cuda().contiguous()


def dirty(words, H, W):
    """ones in the bits past H W of the last word"""
    words = words.copy().view("<u8")
    tail = H * W % 64
    if tail:
        words[:, -1] |= np.uint64(0xFFFFFFFFFFFFFFFF) << np.uint64(tail)
    return words.view(np.int64)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("non_overlap", [False, True], ids=["overlap", "non_overlap"])
def test_histogram_equals_the_host_oracle(shape, non_overlap):
    from sam2_video.kernels import ops
    H, W = shape
    low = planes(H, W)
    v = video_res(low, H, W, non_overlap)
    rng = np.random.default_rng(H * 7 + W)
    gt = rng.random((len(CATS), H, W)) < 0.4
    ones = np.ones((len(CATS), H, W), bool)
    for K in (1, 13, 64):
        cuts = cuts_of(K)
        none = sweep(low, H, W, CATS, cuts, None, non_overlap)
        assert np.array_equal(none, R.np_hist(v, CATS, cuts, None)), K
        assert np.all(none[:, 1] == 0) and np.all(none.sum(axis=(1, 2)) == H * W)
        assert none[1, 0, 0] == H * W  # the empty category: -inf everywhere
        for g in (gt, ones):
            words = ops.pack_mask_bits(g)
            want = R.np_hist(v, CATS, cuts, g)
            assert np.array_equal(sweep(low, H, W, CATS, cuts, words, non_overlap), want), K
            assert np.array_equal(sweep(low, H, W, CATS, cuts, dirty(words, H, W), non_overlap), want), K
            assert np.all(want.sum(axis=(1, 2)) == H * W)


def test_crafted_values_on_and_around_a_cut():
    """planes of one power of two upsample to that constant exactly (the two tap weights sum to 1 within half
    an ulp): a value exactly on a cut and one fp32 step below the next cut, -0.0 against a cut of 0.0, NaN
    (skipped in the maximum; alone it leaves -inf).  +-inf planes (NaN where a tap weight is 0) go through the
    oracle only."""
    H, W = 33, 65
    above_half = np.nextafter(np.float32(0.5), np.float32(1))
    cuts = np.asarray([-2.0, 0.0, 0.0, 0.5, above_half, 2.0], np.float32)
    consts = [0.5, 2.0, -0.0, -2.0, np.nan, -4.0, np.inf, -np.inf]
    n_exact = 6
    low = torch.zeros(len(consts) + 1, 8, 8)
    for i, x in enumerate(consts):
        low[i] = float(x)
    low[-1] = torch.randn(8, 8, generator=torch.Generator().manual_seed(1))
    low = low.cuda().contiguous()
    cats = [[i] for i in range(len(consts))] + [[4, 8], [4, 2], [8, 4, 5], [6, 7]]
    v = video_res(low, H, W)
    for i, x in enumerate(consts[:n_exact]):
        assert np.array_equal(v[i], np.full((H, W), x, np.float32), equal_nan=True), i
    assert np.signbit(v[2]).all()
    got = sweep(low, H, W, cats, cuts)
    assert np.array_equal(got, R.np_hist(v, cats, cuts))
    bins = [int(np.argmax(got[i, 0])) for i in range(n_exact)]
    assert bins == [4, 6, 3, 1, 0, 0]  # (0.5: on its cut, below the next; -0.0 >= 0.0; NaN counts nowhere)
    assert all(got[i, 0, b] == H * W for i, b in enumerate(bins))
    assert np.array_equal(got[9], got[2])  # NaN beside -0.0: the maximum is -0.0
    assert np.array_equal(got[8], got[10])  # NaN and -4 beside the noise plane: the noise plane (> -4) decides
    assert np.all(got.sum(axis=(1, 2)) == H * W)
    # the non-overlap clamp: finite planes only (torch.argmax, the oracle's, lets a NaN win; the kernel skips it)
    fin = low[[0, 1, 2, 3, 5, 8]].contiguous()
    cats2 = [[0], [1], [5], [5, 0], [2, 3, 4]]
    got2 = sweep(fin, H, W, cats2, cuts, non_overlap=True)
    assert np.array_equal(got2, R.np_hist(video_res(fin, H, W, True), cats2, cuts))
    assert np.all(got2.sum(axis=(1, 2)) == H * W)


def test_hist_buffers_are_overwritten_and_runs_are_bit_equal():
    H, W = 33, 65
    low = planes(H, W)
    cuts = cuts_of(13)
    from sam2_video.kernels import ops
    words = ops.pack_mask_bits(np.random.default_rng(2).random((len(CATS), H, W)) < 0.5)
    a = sweep(low, H, W, CATS, cuts, words)
    buf = torch.full((len(CATS), 2, 14), -12345, device="cuda", dtype=torch.int32)
    b = sweep(low, H, W, CATS, cuts, words, hist=buf)
    c = sweep(low, H, W, CATS, cuts, words, hist=buf)  # (and over its own earlier result)
    assert np.array_equal(a, b) and np.array_equal(a, c) and np.array_equal(buf.cpu().numpy(), a)


def test_large_odd_case_against_numpy():
    """64^2 -> 517 x 1031 (521 workgroups, the last word partial), 4 of 5 objects in two categories"""
    from sam2_video.kernels import ops
    g = torch.Generator().manual_seed(11)
    low = (3 * torch.nn.functional.avg_pool2d(torch.randn(5, 1, 64, 64, generator=g), 5, stride=1, padding=2)[:, 0])
    low = low.cuda().contiguous()
    H, W, cats = 517, 1031, [[4, 1], [0, 2]]
    yy, xx = np.mgrid[:H, :W]
    gt = np.stack([(yy // 40 + xx // 60) % 2 == 0, yy > xx // 2])
    for non_overlap in (False, True):
        v = video_res(low, H, W, non_overlap)
        got = sweep(low, H, W, cats, cuts_of(13), dirty(ops.pack_mask_bits(gt), H, W), non_overlap)
        assert np.array_equal(got, R.np_hist(v, cats, cuts_of(13), gt))


def oracle_export(v, cats, cut):
    return [np.logical_or.reduce([v[o] >= cut for o in objs], axis=0) if objs else np.zeros(v.shape[1:], bool)
            for objs in cats]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("non_overlap", [False, True], ids=["overlap", "non_overlap"])
def test_export_at_a_cut(shape, non_overlap):
    from sam2_video.kernels import ops
    H, W = shape
    low = planes(H, W)
    low[0] = 0.25  # a constant plane: every pixel exactly on the cut 0.25 below
    v = video_res(low, H, W, non_overlap)
    off, obj = csr(CATS)
    _, plain_scores = ops.mask_export(low, H, W, off, obj, len(CATS), non_overlap)
    for cut in (0.25, float(TT.logit_cuts([0.35])[0]), float(np.nextafter(np.float32(0.25), np.float32(1))), -11.0):
        bits, scores, vmax = ops.mask_export(low, H, W, off, obj, len(CATS), non_overlap, cut=cut)
        want = np.stack(oracle_export(v, CATS, np.float32(cut)))
        assert np.array_equal(bits.cpu().numpy(), ops.pack_mask_bits(want)), cut
        assert np.array_equal(vmax.cpu().numpy().view(np.int32), v.reshape(13, -1).max(axis=1).view(np.int32))
        assert torch.equal(scores, plain_scores)  # the score does not depend on the cut
        # and through the run-boundary extraction: the RLE of the oracle's mask
        hdr, trans = ops.rle_transitions(bits, H, W)
        hdr, trans = hdr.cpu().numpy(), trans.cpu().numpy()
        for c, m in enumerate(want):
            n, o = int(hdr[c, 0]), int(hdr[c, 1])
            assert rle.from_transitions(trans[o:o + n], H, W) == rle.encode(m) and hdr[c, 2] == m.sum()
    if not non_overlap:
        assert want[0].all()  # (the last cut, -11, admits the constant plane's category entirely)


def test_export_without_a_cut_is_unchanged():
    """the default entry point against the oracle of tests/test_rle_export_gpu.py: `> 0` bits, float64 mean
    sigmoid within 1e-5; then a NaN and a -0.0 plane under both entry points"""
    from sam2_video.kernels import ops
    H, W = 33, 65
    low = planes(H, W)
    off, obj = csr(CATS)

    def positive(v):
        return np.stack([np.logical_or.reduce([v[o] > 0 for o in objs], axis=0) if objs else np.zeros((H, W), bool)
                         for objs in CATS])

    for non_overlap in (False, True):
        v = video_res(low, H, W, non_overlap)
        bits, scores = ops.mask_export(low, H, W, off, obj, len(CATS), non_overlap)
        assert np.array_equal(bits.cpu().numpy(), ops.pack_mask_bits(positive(v)))
        assert np.abs(scores.cpu().numpy() - R.sigmoid64(v).reshape(13, -1).mean(axis=1)).max() <= 1e-5
    low[3] = float("nan")
    low[4] = -0.0
    v = video_res(low, H, W)
    bits, _ = ops.mask_export(low, H, W, off, obj, len(CATS), False)
    assert np.array_equal(bits.cpu().numpy(), ops.pack_mask_bits(positive(v)))
    bits, _, vmax = ops.mask_export(low, H, W, off, obj, len(CATS), False, cut=0.0)
    want = np.stack(oracle_export(v, CATS, np.float32(0)))
    assert np.array_equal(bits.cpu().numpy(), ops.pack_mask_bits(want))
    assert want[3].all() and not want[4].any()  # categories [4] (-0.0 >= 0.0) and [3] (NaN)
    vm = vmax.cpu().numpy()
    assert vm[3] == -np.inf and vm[4] == 0.0
    with pytest.raises(AssertionError):
        ops.mask_export(low, H, W, off, obj, len(CATS), False, vmax=torch.empty(13, device="cuda"))


@pytest.mark.parametrize("shape", [(33, 65), (9, 7)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_counts_equal_the_reference_formulation(shape):
    """torch.sigmoid of the bilinear output on the CPU -> float16 -> `>= thr`, np.any per category: every count
    differs from the sweep's by at most the category's number of ambiguous pixels -- on these seeds none,
    asserted, so the comparison is exact"""
    H, W = shape
    for seed in {(33, 65): (3, 4, 6), (9, 7): (1, 6, 7)}[shape]:  # (seeds whose nearest pixel is > 6 bands away)
        low = (4 * planes(H, W, seed)).contiguous()
        v = video_res(low, H, W)
        amb = R.ambiguous(v, DEFAULT)
        assert not amb.any(), "choose another seed: this one has ambiguous pixels"
        ref = R.reference_pixels(v, DEFAULT)  # [K, N, H, W]
        gt = np.random.default_rng(seed).random((len(CATS), H, W)) < 0.5
        from sam2_video.kernels import ops
        hist = sweep(low, H, W, CATS, TT.logit_cuts(DEFAULT), ops.pack_mask_bits(gt)).astype(np.int64)
        for c, objs in enumerate(CATS):
            for k in range(len(DEFAULT)):
                pred = ref[k][objs].any(axis=0) if objs else np.zeros((H, W), bool)
                assert hist[c, :, k + 1:].sum() == pred.sum(), (seed, c, k)
                assert hist[c, 1, k + 1:].sum() == (pred & gt[c]).sum(), (seed, c, k)
            assert hist[c, 1].sum() == gt[c].sum()


def test_sweep_in_a_hip_graph():
    """capturable: no scratch but the caller's, one stream"""
    from sam2_video.kernels import ops
    H, W = 33, 65
    a = planes(H, W)
    b = (-a).flip(0).contiguous()
    off, obj = csr(CATS)
    cuts = torch.from_numpy(cuts_of(13)).cuda()
    static_in = a.clone()
    ops.mask_sweep(static_in, H, W, off, obj, len(CATS), cuts)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        hist = ops.mask_sweep(static_in, H, W, off, obj, len(CATS), cuts)
        _, _, vmax = ops.mask_export(static_in, H, W, off, obj, len(CATS), False, cut=0.5)
    for x in (b, a):
        static_in.copy_(x)
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(hist.cpu().numpy(), sweep(x, H, W, CATS, cuts_of(13)))
        assert torch.equal(vmax, ops.mask_export(x, H, W, off, obj, len(CATS), False, cut=0.5)[2])


def test_arguments_outside_the_limits_are_refused():
    from sam2_video.kernels import _lib, ops
    low = torch.zeros(1, 8, 8, device="cuda")
    off, obj = csr([[0]])
    hist = torch.zeros(1, 2, 66, device="cuda", dtype=torch.int32)
    cuts = torch.zeros(65, device="cuda")
    for K in (0, 65):  # 1 <= K <= 64
        with pytest.raises(_lib.HipKernelError):
            _lib.call("s2h_mask_sweep", 1, 8, 8, 8, 8, low.data_ptr(), 1, off.data_ptr(), obj.data_ptr(), 0, K,
                      cuts.data_ptr(), None, hist.data_ptr(), None)
    with pytest.raises(_lib.HipKernelError):  # H W > 2^24
        _lib.call("s2h_mask_sweep", 1, 8, 8, 4097, 4096, low.data_ptr(), 1, off.data_ptr(), obj.data_ptr(), 0, 1,
                  cuts.data_ptr(), None, hist.data_ptr(), None)
    with pytest.raises(_lib.HipKernelError):
        _lib.call("s2h_mask_export_cut", 1, 8, 8, 4097, 4096, low.data_ptr(), 1, off.data_ptr(), obj.data_ptr(), 0,
                  0.0, hist.data_ptr(), low.data_ptr(), low.data_ptr(), low.data_ptr(), None)
    with pytest.raises(AssertionError):
        ops.mask_sweep(low, 8, 8, off, obj, 1, cuts)
