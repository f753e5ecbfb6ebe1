"""Shared inputs and scipy references of the connected-components / hole-filling tests
(test_cc_host.py runs the host build of the union-find header on them, test_cc_gpu.py the kernels)."""
import functools

import numpy as np
import torch

# 65 x 130 straddles every tile edge (a wave covers 64 consecutive pixels, rows are not a multiple of it)
SHAPES = [(1, 1), (1, 17), (17, 1), (2, 2), (37, 53), (64, 64), (65, 130), (128, 128), (256, 256)]
BATCHES = [1, 3, 13]
NOISE = [(p, seed) for p in (0.3, 0.5, 0.59, 0.9) for seed in (0, 1, 2)]


def _serpentine(H, W):
    """full rows on even lines joined by one pixel at alternating ends on odd lines: one chain of about
    H * W / 2 pixels, the deepest propagation there is"""
    m = np.zeros((H, W), bool)
    m[0::2] = True
    for k, y in enumerate(range(1, H, 2)):
        m[y, W - 1 if k % 2 == 0 else 0] = True
    return m


def _spiral(H, W):
    m = np.zeros((H, W), bool)
    y = x = 0
    dy, dx = 0, 1
    m[0, 0] = True
    while True:
        moved = False
        for _ in range(2):  # straight on, else one turn to the right
            ny, nx, ay, ax = y + dy, x + dx, y + 2 * dy, x + 2 * dx
            if 0 <= ny < H and 0 <= nx < W and not m[ny, nx] and not (0 <= ay < H and 0 <= ax < W and m[ay, ax]):
                y, x = ny, nx
                m[y, x] = True
                moved = True
                break
            dy, dx = dx, -dy
        if not moved:
            return m


def _rings(H, W):
    """one-pixel rectangular rings two apart: nested, not connected"""
    m = np.zeros((H, W), bool)
    for d in range(0, (min(H, W) + 1) // 2, 3):
        m[d, d:W - d] = m[H - 1 - d, d:W - d] = True
        m[d:H - d, d] = m[d:H - d, W - 1 - d] = True
    return m


def _corner_blocks(H, W, b=6):
    """around (32, 32), (64, 64) and the centre: the upper-left and lower-right b x b blocks set, the other
    two clear -- each pair touches only at the shared corner"""
    m = np.zeros((H, W), bool)
    for cy, cx in ((32, 32), (64, 64), (H // 2, W // 2)):
        if cy < H and cx < W:
            m[max(cy - b, 0):cy, max(cx - b, 0):cx] = True
            m[cy:cy + b, cx:cx + b] = True
    return m


@functools.lru_cache(maxsize=None)
def patterns(H, W):
    """name -> bool [H, W]"""
    yy, xx = np.mgrid[0:H, 0:W]
    out = {
        "all_background": np.zeros((H, W), bool),
        "all_foreground": np.ones((H, W), bool),
        "checkerboard": (yy + xx) % 2 == 0,
        "anti_diagonal": yy + xx == min(H, W) - 1,
        "main_diagonal": yy == xx,
        "serpentine": _serpentine(H, W),
        "spiral": _spiral(H, W),
        "rings": _rings(H, W),
        "corner_blocks": _corner_blocks(H, W),
    }
    for p, seed in NOISE:
        out[f"noise_p{p}_s{seed}"] = np.random.default_rng(seed).random((H, W)) < p
    return out


def scores_of(mask):
    """fp32 scores whose > 0 set is `mask`: +-(1 .. 2), with exact +0.0 and -0.0 on part of the background"""
    H, W = mask.shape
    mag = 1.0 + ((np.arange(H * W).reshape(H, W) * 7) % 16) / 16.0
    s = np.where(mask, mag, -mag).astype(np.float32)
    zero = ~mask & ((np.arange(H * W).reshape(H, W) % 5) == 0)
    s[zero] = np.where((np.arange(H * W).reshape(H, W) % 2) == 0, 0.0, -0.0).astype(np.float32)[zero]
    return s


def reference(binary):
    """scipy 8-connected labelling made canonical: (1 + smallest row-major index of the component, its
    area), both 0 on the background; int32 [H, W]"""
    from scipy import ndimage
    lab, n = ndimage.label(binary, structure=np.ones((3, 3), dtype=np.int32))
    if n == 0:
        z = np.zeros(binary.shape, np.int32)
        return z, z.copy()
    idx = np.arange(binary.size).reshape(binary.shape)
    first = np.asarray(ndimage.minimum(idx, lab, index=np.arange(1, n + 1))).astype(np.int64)
    canon = np.where(lab > 0, first[np.maximum(lab, 1) - 1] + 1, 0)
    areas = np.bincount(lab.ravel(), minlength=n + 1)[lab] * (lab > 0)
    return canon.astype(np.int32), areas.astype(np.int32)


@functools.lru_cache(maxsize=None)
def shape_case(H, W):
    """every pattern of a shape: (names, scores [P, H, W] fp32, {positive: (labels, areas) int32 [P, H, W]});
    computed once, shared by the tests, read-only"""
    pats = patterns(H, W)
    names = list(pats)
    scores = np.stack([scores_of(pats[k]) for k in names])
    ref = {}
    for positive in (True, False):
        r = [reference(s > 0 if positive else s <= 0) for s in scores]
        ref[positive] = (np.stack([a for a, _ in r]), np.stack([b for _, b in r]))
        for a in ref[positive]:
            a.setflags(write=False)
    scores.setflags(write=False)
    return names, scores, ref


def chunks(P, N):
    """index lists of N different patterns each that together cover 0..P-1 (the last one wraps)"""
    return [[(s + j) % P for j in range(N)] for s in range(0, P, N)] if N <= P else [[j % P for j in range(N)]]


# ------------------------------------------------------------------------------------ hole filling
MAX_AREAS = [1, 8, 64]


def _host_cases():
    """the three inputs of tests/test_predictor_host.py::test_fill_holes_and_remove_sprinkles"""
    m = -torch.ones(1, 1, 20, 20)
    m[0, 0, 2:12, 2:12] = 3.0
    m[0, 0, 5:7, 5:7] = -2.0
    m[0, 0, 15, 15] = 5.0
    m[0, 0, 9:12, 14:18] = -3.0
    m2 = m.clone()
    m2[0, 0, 4:8, 4:8] = -2.0
    m3 = -torch.ones(1, 1, 6, 6)
    m3[0, 0, 1, 1] = m3[0, 0, 2, 2] = 1.0
    return {"host_object_hole_sprinkle": m, "host_large_hole": m2, "host_diagonal": m3}


def ordering_case():
    """7 x 7 of -2 with a 3 x 3 block of +1 whose centre is -1.  At max_area 8 the centre is filled first
    (-> 0.1); the ring then has area 9 > 8 and stays.  Two passes from one snapshot would remove the ring."""
    m = torch.full((1, 1, 7, 7), -2.0)
    m[0, 0, 2:5, 2:5] = 1.0
    m[0, 0, 3, 3] = -1.0
    return m


def _smooth(N, S, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, 1, S, S, generator=g)
    return torch.nn.functional.avg_pool2d(x, 5, stride=1, padding=2)


def _zeros_field(seed):
    """a smooth field with exact 0.0 and -0.0 sprinkled in: both are background"""
    x = _smooth(3, 48, seed).clone()
    g = torch.Generator().manual_seed(seed + 1)
    r = torch.rand(x.shape, generator=g)
    x[r < 0.15] = 0.0
    x[(r >= 0.15) & (r < 0.3)] = -0.0
    return x


@functools.lru_cache(maxsize=None)
def fill_inputs():
    """name -> fp32 [N, 1, H, W] (CPU)"""
    out = dict(_host_cases())
    out["ordering"] = ordering_case()
    out["zeros"] = _zeros_field(7)
    for S in (64, 128, 256):
        out[f"smooth{S}"] = _smooth(13, S, S)
    return out


@functools.lru_cache(maxsize=None)
def fill_reference(name, max_area):
    """the host (scipy) path of the predictor on a CPU tensor: the oracle"""
    from sam2_video.predictor import fill_holes_in_mask_scores
    x = fill_inputs()[name]
    assert not x.is_cuda
    return fill_holes_in_mask_scores(x.clone(), max_area)
