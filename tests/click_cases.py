"""Cases and independent numpy models for the correction clicks (csrc/clicks.h, csrc/clicks.hip,
sam2_video/model/modeling/sam2_utils.py), shared by test_clicks_host.py and test_clicks_gpu.py.

Two models of D2, the exact squared Euclidean distance transform with the ring just outside the image counted as
background: d2_brute compares every pixel with every clear pixel of the padded mask (shapes up to 24 x 24), and
d2_separable takes row distances from running maxima / minima of the clear positions and then scans the rows
above and below.  Neither shares code with the package; where scipy imports, rint(distance_transform_edt^2) of
the padded mask is a third."""
import numpy as np

SHAPES = [(1, 1), (1, 70), (67, 3), (5, 64), (65, 130), (96, 200)]
BRUTE_MAX = 24


# ------------------------------------------------------------------------------------------------ models
def d2_brute(m):
    m = np.asarray(m, bool)
    H, W = m.shape
    assert H <= BRUTE_MAX and W <= BRUTE_MAX
    padded = np.zeros((H + 2, W + 2), bool)
    padded[1:-1, 1:-1] = m
    cy, cx = np.nonzero(~padded)
    yy, xx = np.mgrid[1:H + 1, 1:W + 1]
    d = (yy[..., None] - cy) ** 2 + (xx[..., None] - cx) ** 2
    return np.where(m, d.min(axis=-1), 0).astype(np.int64)


def row_dist(m):
    """per pixel the distance along its row to the nearest clear position, -1 and W counting as clear"""
    m = np.asarray(m, bool)
    H, W = m.shape
    x = np.arange(W)[None]
    last = np.maximum.accumulate(np.where(m, -1, x), axis=1)
    nxt = np.minimum.accumulate(np.where(m, W, x)[:, ::-1], axis=1)[:, ::-1]
    return np.minimum(x - last, nxt - x).astype(np.int64)


def d2_separable(m):
    m = np.asarray(m, bool)
    H, W = m.shape
    h2 = np.zeros((H + 2, W), np.int64)  # rows -1 and H: distance 0
    h2[1:-1] = row_dist(m) ** 2
    best = h2[1:-1].copy()
    for d in range(1, H + 1):
        if d * d >= best.max():
            break
        up = h2[max(0, 1 - d):H + 1 - d]
        up = np.concatenate([np.zeros((H - len(up), W), np.int64), up])       # rows above -1 never win: see below
        down = h2[1 + d:H + 2]
        down = np.concatenate([down, np.zeros((H - len(down), W), np.int64)])
        # a row beyond -1 or H is entered as distance 0 at d^2, which is larger than the (d - 1)^2 or less that
        # the border row itself gave, so it changes nothing
        best = np.minimum(best, d * d + np.minimum(up, down))
    return best


def d2_scipy(m):
    from scipy import ndimage
    e = ndimage.distance_transform_edt(np.pad(np.asarray(m, bool), 1))[1:-1, 1:-1]
    return np.rint(e * e).astype(np.int64)


def d2_model(m):
    m = np.asarray(m, bool)
    return d2_brute(m) if max(m.shape) <= BRUTE_MAX else d2_separable(m)


def center_model(gt, pred, d2=d2_model):
    """-> ((x, y), label, (dn, dp)) of one object"""
    gt = np.asarray(gt, bool)
    pred = np.zeros_like(gt) if pred is None else np.asarray(pred, bool)
    dn_map, dp_map = d2(gt & ~pred).reshape(-1), d2(~gt & pred).reshape(-1)
    i_n, i_p = int(np.argmax(dn_map)), int(np.argmax(dp_map))
    dn, dp = int(dn_map[i_n]), int(dp_map[i_p])
    label = int(dn > dp)
    idx = i_n if label else i_p
    W = gt.shape[1]
    return (idx % W, idx // W), label, (dn, dp)


def regions(gt, pred):
    """-> (R0, R1) of the uniform sampler"""
    gt = np.asarray(gt, bool)
    pred = np.zeros_like(gt) if pred is None else np.asarray(pred, bool)
    all_correct = bool((gt == pred).all())
    return (~gt & pred) | (all_correct & ~gt), gt & ~pred


def uniform_model(gt, pred, r):
    """r: ints in [0, 2^32) -> (points [P, 2], labels [P], (|R0|, |R1|)) of one object"""
    r0, r1 = regions(gt, pred)
    flat = np.flatnonzero((r0 | r1).reshape(-1))
    n, W = len(flat), r0.shape[1]
    points, labels = [], []
    for v in r:
        if n == 0:
            points.append((0, 0))
            labels.append(0)
            continue
        q = int(flat[(int(v) * n) >> 32])
        points.append((q % W, q // W))
        labels.append(int(r1.reshape(-1)[q]))
    return np.asarray(points, np.float32).reshape(-1, 2), np.asarray(labels, np.int32), (int(r0.sum()), int(r1.sum()))


def draws_for(gt, pred):
    """the draws that matter for one object: 0, 2^32 - 1, and the smallest and the largest draw that land on the
    first and on the last pixel of each of the two sets"""
    r0, r1 = regions(gt, pred)
    union = (r0 | r1).reshape(-1)
    n = int(union.sum())
    out = [0, 2 ** 32 - 1]
    if n == 0:
        return out
    rank_of = np.cumsum(union) - 1
    for s in (r0, r1):
        pos = np.flatnonzero(s.reshape(-1))
        if len(pos) == 0:
            continue
        for q in (pos[0], pos[-1]):
            k = int(rank_of[q])
            out += [-((-k * 2 ** 32) // n), -((-(k + 1) * 2 ** 32) // n) - 1]  # ceil(k 2^32 / n), ceil((k + 1) 2^32 / n) - 1
    assert all(0 <= v < 2 ** 32 for v in out)
    return out


# ------------------------------------------------------------------------------------------------ patterns
def disc(H, W, cy, cx, rad):
    yy, xx = np.mgrid[0:H, 0:W]
    return (yy - cy) ** 2 + (xx - cx) ** 2 <= rad * rad


def mask_patterns(H, W, seed=0):
    """{name: bool [H, W]}"""
    rng = np.random.default_rng(1000 * H + W + seed)
    out = {"empty": np.zeros((H, W), bool), "full": np.ones((H, W), bool)}
    one = np.zeros((H, W), bool)
    one[H // 2, W // 3] = True
    out["one_set"] = one
    hole = np.ones((H, W), bool)
    hole[H // 3, W // 2] = False
    out["one_clear"] = hole
    yy, xx = np.mgrid[0:H, 0:W]
    out["checker"] = (yy + xx) % 2 == 0
    for name, sl in (("top", np.s_[:max(1, H // 3), :]), ("bottom", np.s_[H - max(1, H // 3):, :]),
                     ("left", np.s_[:, :max(1, W // 3)]), ("right", np.s_[:, W - max(1, W // 3):])):
        m = np.zeros((H, W), bool)
        m[sl] = True
        out[name] = m
    inner = np.zeros((H, W), bool)
    inner[1:H - 1, 1:W - 1] = True  # touches no border (empty on a 1- or 2-pixel side)
    out["inner"] = inner
    rad = max(0, (min(H, W) - 3) // 2)
    out["disc"] = disc(H, W, H // 2, W // 2, rad)
    r2 = max(0, (min(H, W // 2) - 3) // 2)
    out["two_discs"] = disc(H, W, H // 2, W // 4, r2) | disc(H, W, H // 2, W // 4 + W // 2, r2)
    last = np.zeros((H, W), bool)
    last[H - 1, W - 1] = True
    out["last_pixel"] = last
    for p in (0.3, 0.7, 0.95, 1.0):
        out[f"random{p}"] = rng.random((H, W)) <= p if p < 1.0 else np.ones((H, W), bool)
    blobs = np.zeros((H, W), bool)
    for _ in range(4):
        blobs |= disc(H, W, rng.integers(0, H), rng.integers(0, W), rng.integers(1, max(2, min(H, W) // 2 + 1)))
    out["blobs"] = blobs
    return out


def pair_patterns(H, W):
    """{name: (gt bool [H, W], pred bool [H, W] or None)}"""
    m = mask_patterns(H, W)
    out = {}
    for name in ("empty", "full", "one_set", "one_clear", "checker", "disc", "two_discs", "last_pixel", "blobs"):
        out[f"{name}/absent"] = (m[name], None)             # pred absent: FN = gt
        out[f"{name}/fp"] = (np.zeros((H, W), bool), m[name])  # FP = the mask
    for name in ("top", "bottom", "left", "right", "inner", "random0.7"):
        out[f"{name}/absent"] = (m[name], None)
    # FN and FP mirror images of each other: equal maxima, so label 0 and the FP point
    half = np.zeros((H, W), bool)
    if W >= H:
        half[:, :W // 2] = m["blobs"][:, :W // 2] | m["disc"][:, :W // 2]
        mirror = half[:, ::-1]
    else:
        half[:H // 2] = m["blobs"][:H // 2] | m["disc"][:H // 2]
        mirror = half[::-1]
    out["mirror"] = (half, mirror.copy())
    out["mirror_swapped"] = (mirror.copy(), half)
    out["correct_with_background"] = (m["blobs"], m["blobs"].copy())
    out["correct_empty"] = (m["empty"], m["empty"].copy())
    out["correct_full"] = (m["full"], m["full"].copy())
    out["shifted"] = (m["blobs"], np.roll(m["blobs"], (1, 2), (0, 1)))
    out["random"] = (m["random0.7"], m["random0.3"])
    out["fn_beats_fp"] = (m["disc"], m["one_set"] & ~m["disc"])
    return out
