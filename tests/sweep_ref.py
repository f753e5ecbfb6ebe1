"""numpy oracles the threshold-sweep tests share (no test in here): the histogram s2h_mask_sweep must give,
the ambiguous band of the float16 thresholding, and the reference's own formulation of a thresholded mask."""
import numpy as np
import torch


def sigmoid64(v):
    return 1.0 / (1.0 + np.exp(-np.asarray(v, dtype=np.float64)))


def merged_max(v, objs):
    """maximum over the category's objects of v [N, H, W], NaN skipped, -inf without objects"""
    m = np.full(v.shape[1:], -np.inf, dtype=np.float32)
    for o in objs:
        m = np.fmax(m, v[o])
    return m


def np_hist(v, cats, cuts, gt=None):
    """v [N, H, W] fp32 final values, cats: object lists, cuts fp32 [K], gt bool [ncat, H, W] or None
    -> int32 [ncat, 2, K + 1]: hist[c][g][b] = #pixels with ground-truth bit g and b = #{k : m >= cuts[k]}"""
    cuts = np.asarray(cuts, dtype=np.float32)
    K = cuts.size
    hist = np.zeros((len(cats), 2, K + 1), dtype=np.int32)
    for c, objs in enumerate(cats):
        m = merged_max(v, objs)
        b = (m[..., None] >= cuts).sum(axis=-1)
        g = np.zeros(b.shape, bool) if gt is None else np.asarray(gt[c], bool)
        for bit in (0, 1):
            hist[c, bit] = np.bincount(b[g == bool(bit)].ravel(), minlength=K + 1)
    return hist


def ambiguous(v, thresholds):
    """bool [K, *v.shape]: |sigmoid64(v) - mid(t)| <= 2^-22, where float32 sigmoid -> float16 -> `>=` may land
    on either side of v >= cut(t)"""
    from sam2_video.eval.tune_threshold import AMBIGUOUS_BAND, threshold_mid
    p = sigmoid64(v)
    return np.stack([np.abs(p - threshold_mid(t)[0]) <= AMBIGUOUS_BAND for t in thresholds])


def reference_pixels(v, thresholds):
    """the reference's formulation, bool [K, *v.shape]: torch.sigmoid in fp32 on the CPU -> float16 -> `>= thr`"""
    probs = torch.sigmoid(torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32))).numpy().astype(np.float16)
    return np.stack([probs >= np.float16(t) for t in thresholds])  # (what `float16 array >= float` compares)


def cut_pixels(v, thresholds):
    """the feature's contract, bool [K, *v.shape]: v >= cut(t)"""
    from sam2_video.eval.tune_threshold import logit_cuts
    return np.stack([np.asarray(v, np.float32) >= c for c in logit_cuts(thresholds)])
