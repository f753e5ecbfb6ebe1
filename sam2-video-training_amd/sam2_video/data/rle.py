"""COCO run-length-encoded masks without pycocotools (not installed here).

The reference decodes annotation masks with pycocotools' `mask.decode` (dataset.py:123-137).  This
restates the published COCO RLE format it reads:
  * a mask [h, w] is flattened column-major (Fortran order) and described by alternating run
    lengths of 0s and 1s, starting with 0s;
  * the compressed string form (`counts` as str) stores each run length as a little-endian
    sequence of 5-bit groups, one character (group + 48) per group, bit 0x20 = "more groups
    follow", bit 0x10 of the last group = sign; from the 4th count on the value is the
    difference to the count two places earlier.
Host-side numpy, once per annotation (the reference caches decoded masks per image too).
"""
from __future__ import annotations

import ast
from typing import Dict, List, Union

import numpy as np


def counts_from_string(s: str) -> List[int]:
    cnts: List[int] = []
    p, n = 0, len(s)
    while p < n:
        x, k, more = 0, 0, 1
        while more:
            c = ord(s[p]) - 48
            x |= (c & 0x1F) << (5 * k)
            more = c & 0x20
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(cnts) > 2:
            x += cnts[-2]
        cnts.append(x)
    return cnts


def counts_to_string(cnts: List[int]) -> str:
    # all counts at once, one 5-bit group per pass (an int64 has at most 13): a frame's export encodes tens
    # of thousands of runs, once per category
    orig = np.asarray(cnts, dtype=np.int64).reshape(-1)
    x = orig.copy()
    if x.size > 3:
        x[3:] -= orig[1:-2]
    chars = np.zeros((x.size, 13), dtype=np.uint8)
    used = np.zeros((x.size, 13), dtype=bool)
    alive = np.ones(x.size, dtype=bool)
    for k in range(13):
        if not alive.any():
            break
        c = x & 0x1F
        x = x >> 5
        more = np.where((c & 0x10) != 0, x != -1, x != 0) & alive
        chars[:, k] = (c | (more.astype(np.int64) << 5)) + 48
        used[:, k] = alive
        alive = more
    return chars[used].tobytes().decode("ascii")


def _as_rle(rle: Union[Dict, str]) -> Dict:
    if isinstance(rle, str):  # some exports store the dict's repr (data/endovis18.json)
        rle = ast.literal_eval(rle)
    if not isinstance(rle, dict) or "counts" not in rle or "size" not in rle:
        raise ValueError("expected an RLE dict {'size': [h, w], 'counts': ...} (polygons are not supported)")
    return rle


def counts_of(rle: Union[Dict, str]):
    """RLE dict (compressed or uncompressed counts) -> (h, w, run lengths as a list)"""
    rle = _as_rle(rle)
    h, w = (int(v) for v in rle["size"])
    cnts = rle["counts"]
    if isinstance(cnts, bytes):
        cnts = cnts.decode("ascii")
    if isinstance(cnts, str):
        cnts = counts_from_string(cnts)
    return h, w, list(cnts)


def decode(rle: Union[Dict, str]) -> np.ndarray:
    """RLE (compressed or uncompressed counts) -> uint8 mask [h, w]"""
    h, w, cnts = counts_of(rle)
    cnts = np.asarray(cnts, dtype=np.int64)
    if cnts.sum() != h * w:
        raise ValueError(f"RLE counts cover {int(cnts.sum())} pixels, mask has {h * w}")
    vals = np.zeros(len(cnts), dtype=np.uint8)
    vals[1::2] = 1
    flat = np.repeat(vals, cnts)
    return flat.reshape(w, h).T.copy()  # column-major


def encode(mask: np.ndarray) -> Dict:
    """uint8/bool mask [h, w] -> compressed RLE dict"""
    m = np.asarray(mask).astype(bool)
    h, w = m.shape
    flat = m.T.reshape(-1)
    change = np.flatnonzero(flat[1:] != flat[:-1]) + 1
    bounds = np.concatenate([[0], change, [flat.size]])
    runs = np.diff(bounds).tolist()
    if flat.size and flat[0]:
        runs = [0] + runs
    return {"size": [h, w], "counts": counts_to_string(runs)}


def counts_from_transitions(trans, n_pixels: int) -> List[int]:
    """run lengths from run boundaries: `trans` are the ascending positions j in [0, n_pixels) of the
    column-major flattened mask with m[j] != m[j - 1] (m[-1] = 0), as s2h_rle_transitions writes them; the
    counts are the differences of [0, *trans, n_pixels].  A mask whose first pixel is set has trans[0] == 0
    and so a first count of 0, as pycocotools writes it."""
    t = np.asarray(trans, dtype=np.int64).reshape(-1)
    bounds = np.concatenate([[0], t, [int(n_pixels)]])
    return np.diff(bounds).tolist()


def from_transitions(trans, h: int, w: int) -> Dict:
    """run boundaries of an [h, w] mask -> compressed RLE dict (the dict `encode` gives for that mask)"""
    return {"size": [int(h), int(w)], "counts": counts_to_string(counts_from_transitions(trans, int(h) * int(w)))}


_GRID_POS: Dict = {}


def grid_positions(H: int, rows, cols) -> np.ndarray:
    """the column-major positions c * H + r of a sampling grid (rows x cols of an image of height H), sorted;
    kept per grid (a dataset has one or two)"""
    rows = np.ascontiguousarray(rows, dtype=np.int64)
    cols = np.ascontiguousarray(cols, dtype=np.int64)
    key = (int(H), rows.tobytes(), cols.tobytes())
    pos = _GRID_POS.get(key)
    if pos is None:
        if len(_GRID_POS) >= 16:
            _GRID_POS.clear()
        pos = np.sort((cols[:, None] * int(H) + rows[None, :]).reshape(-1))
        _GRID_POS[key] = pos
    return pos


def runs_hit_grid(run_end, H: int, rows, cols) -> bool:
    """does any sampled position c * H + r (r in rows, c in cols) of a mask of height H fall in a set run?
    run_end: the cumulative sums of the mask's counts (ops.rle_runs); run k covers [run_end[k - 1], run_end[k])
    and the odd runs are set.  Decided from the runs alone: two searches in the sorted positions per mask."""
    end = np.asarray(run_end, dtype=np.int64).reshape(-1)
    if end.size < 2:
        return False
    pos = grid_positions(H, rows, cols)
    lo = np.searchsorted(pos, end[0:-1:2], side="left")  # starts of the set runs 1, 3, ...
    hi = np.searchsorted(pos, end[1::2], side="left")
    return bool((hi > lo[:hi.size]).any())


def area(rle) -> int:
    return int(decode(rle).sum())


def to_bbox(rle) -> List[float]:
    """[x, y, w, h] of the mask's nonzero pixels (pycocotools toBbox semantics)"""
    m = decode(rle)
    ys, xs = np.nonzero(m)
    if ys.size == 0:
        return [0.0, 0.0, 0.0, 0.0]
    return [float(xs.min()), float(ys.min()), float(xs.max() - xs.min() + 1), float(ys.max() - ys.min() + 1)]
