"""Cases of the offline scoring's pair counts (s2h_rle_pair_counts, csrc/pair_counts.h), shared by the host run of
the header (test_pair_counts_host.py) and the kernel (test_pair_counts_gpu.py), and their reference: numpy
rle.decode of every annotation, OR per side, four sums.

A case is {"H", "W", "dt": G lists of COCO counts lists, "gt": the same}.  Sizes: 1 x 1, 1 x 64 (exactly one word),
5 x 13 (65 positions: one bit into a second word), 67 x 61 and 300 x 217 (several workgroups, a partial last word).
Group kinds: an empty predicted side, an empty ground-truth side, both empty (zeros), three overlapping
annotations on one side, an annotation whose first run has length zero (the mask starts set), a single-run
annotation (an empty mask), a full mask, and plain random masks.  G = 1 (every kind at every size) and G = 37 (the
kinds in turn)."""
import numpy as np

from sam2_video.data import rle

SIZES = [(1, 1), (1, 64), (5, 13), (67, 61), (300, 217)]
KINDS = ["empty_dt", "empty_gt", "both_empty", "three_overlapping", "zero_first_run", "single_run", "full", "random"]


def _counts(mask):
    return rle.counts_of(rle.encode(mask))[2]


def _blob(rng, H, W):
    """a random rectangle with random holes (at least the rectangle's corner pixel stays likely set)"""
    y0, x0 = int(rng.integers(0, H)), int(rng.integers(0, W))
    y1, x1 = int(rng.integers(y0, H)) + 1, int(rng.integers(x0, W)) + 1
    m = np.zeros((H, W), bool)
    m[y0:y1, x0:x1] = rng.random((y1 - y0, x1 - x0)) < 0.8
    return m


def _group(kind, rng, H, W):
    """-> (predicted counts lists, ground-truth counts lists) of one group"""
    a, b = _counts(_blob(rng, H, W)), _counts(_blob(rng, H, W))
    if kind == "empty_dt":
        return [], [b]
    if kind == "empty_gt":
        return [a], []
    if kind == "both_empty":
        return [], []
    if kind == "three_overlapping":
        base = _blob(rng, H, W)
        three = [_counts(base), _counts(base | _blob(rng, H, W)), _counts(_blob(rng, H, W))]
        return (three, [b]) if rng.integers(2) else ([a], three)
    if kind == "zero_first_run":
        m = _blob(rng, H, W)
        m[0, 0] = True
        c = _counts(m)
        assert c[0] == 0
        return [c], [b]
    if kind == "single_run":
        return [[H * W]], [b, [H * W]]
    if kind == "full":
        return [[0, H * W]], [b]
    return [a], [b]


def make_cases():
    cases = []
    for si, (H, W) in enumerate(SIZES):
        rng = np.random.default_rng(100 + si)
        for kind in KINDS[:-1]:
            dt, gt = _group(kind, rng, H, W)
            cases.append({"H": H, "W": W, "dt": [dt], "gt": [gt], "name": f"{H}x{W}-G1-{kind}"})
        groups = [_group(KINDS[g % len(KINDS)], rng, H, W) for g in range(37)]
        cases.append({"H": H, "W": W, "dt": [g[0] for g in groups], "gt": [g[1] for g in groups],
                      "name": f"{H}x{W}-G37"})
    return cases


def reference(case):
    """int64 [G, 4]: |p & g|, |p | g|, |p|, |g| by decoding every annotation"""
    H, W = case["H"], case["W"]
    out = np.zeros((len(case["dt"]), 4), np.int64)
    for g, (dt, gt) in enumerate(zip(case["dt"], case["gt"])):
        sides = []
        for anns in (dt, gt):
            m = np.zeros((H, W), bool)
            for c in anns:
                m |= rle.decode({"size": [H, W], "counts": c}).astype(bool)
            sides.append(m)
        p, q = sides
        out[g] = [(p & q).sum(), (p | q).sum(), p.sum(), q.sum()]
    return out
