"""A/B of one round of correction-click sampling: the device path (csrc/clicks.hip) against the host twin of
model/modeling/sam2_utils.py (numpy / scipy, with the copies to the host it needs -- what the reference's
samplers pay), in one process.  Three inputs: 13 objects at 512 x 512 (slanted bars against themselves shifted
and eroded), the two largest annotations of tests/golden/rle_endovis18_sample.json at 1024 x 1280, as in
tests/test_clicks_gpu.py, and the 13 objects once more without a prediction (the first click).  Times are device
events over `--iters` calls after `--warmup` calls, the median and the minimum per call; "kernels" is
ops.error_center_click / ops.error_uniform_click alone on byte masks that are already there, "sampler" the whole
get_next_point call.

    python tools/clicks_ab.py [--iters 20] [--warmup 3]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sam2-video-training_amd"))


def bars(B, H, W, rng):
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.zeros((B, H, W), bool)
    for b in range(B):
        cy, cx, a = rng.integers(H // 4, 3 * H // 4), rng.integers(W // 4, 3 * W // 4), rng.uniform(-1.2, 1.2)
        d = (yy - cy) * np.cos(a) - (xx - cx) * np.sin(a)
        along = (yy - cy) * np.sin(a) + (xx - cx) * np.cos(a)
        out[b] = (np.abs(d) < rng.integers(H // 40 + 2, H // 8)) & (np.abs(along) < rng.integers(H // 6, H // 2))
    return out


def golden_pair():
    from sam2_video.data import rle
    found = []

    def walk(node):
        if isinstance(node, dict):
            if "counts" in node and "size" in node:
                found.append(node)
                return
            node = list(node.values())
        if isinstance(node, list):
            for v in node:
                walk(v)

    with open(os.path.join(ROOT, "tests", "golden", "rle_endovis18_sample.json")) as f:
        walk(json.load(f))
    masks = sorted((rle.decode(a) for a in found), key=lambda m: -int(m.sum()))[:2]
    return np.stack(masks).astype(bool)


def timed(fn, iters, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch
    from sam2_video.kernels import ops
    from sam2_video.model.modeling import sam2_utils as U
    rng = np.random.default_rng(3)
    thirteen = bars(13, 512, 512, rng)
    # (name, ground truth, whether there is a prediction: without one the whole object is the error region, the
    # widest regions and so the longest column scans this input can give)
    cases = [("13 x 512 x 512", thirteen, True), ("2 x 1024 x 1280", golden_pair(), True),
             ("13 x 512 x 512, no prediction", thirteen, False)]
    print(f"correction clicks, one round; {torch.cuda.get_device_name(0)}; median / min ms over {args.iters} calls")
    for name, gt_np, with_pred in cases:
        gt = torch.from_numpy(gt_np).cuda()[:, None]
        B, _, H, W = gt.shape
        shifted = torch.roll(gt, (3, -5), (2, 3)).reshape(B, H, W).contiguous().view(torch.uint8)
        pred = ops.morph_rect(shifted, "erode", (-2, 2), (-1, 1)).view(torch.bool)[:, None] if with_pred else None
        gt8 = gt.reshape(B, H, W).view(torch.uint8)
        pred8 = pred.reshape(B, H, W).view(torch.uint8) if with_pred else None
        r = torch.randint(0, 2 ** 32, (B, 1), dtype=torch.int64, device="cuda")
        err = int((gt != pred).sum()) if with_pred else int(gt.sum())
        _, _, dmax = ops.error_center_click(gt8, pred8)
        print(f"{name}: {err} error pixels, largest squared distance {int(dmax.max())}")
        for method, kernels in (("center", lambda: ops.error_center_click(gt8, pred8)),
                                ("uniform", lambda: ops.error_uniform_click(gt8, pred8, r))):
            rows = {"kernels": timed(kernels, args.iters, args.warmup)}
            for on_device in (True, False):
                gen = torch.Generator(device="cuda").manual_seed(1)
                rows["device sampler" if on_device else "host twin"] = timed(
                    lambda: U.get_next_point(gt, pred, method, generator=gen, on_device=on_device),
                    args.iters if on_device else max(3, args.iters // 4), args.warmup if on_device else 1)
            a = U.get_next_point(gt, pred, method, generator=torch.Generator(device="cuda").manual_seed(1))
            b = U.get_next_point(gt, pred, method, generator=torch.Generator(device="cuda").manual_seed(1),
                                 on_device=False)
            same = bool(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]))
            share = 100.0 * rows["kernels"][0] / rows["device sampler"][0]
            print(f"  {method:8}" + "".join(f" {k} {v[0]:8.3f} / {v[1]:8.3f} ms;" for k, v in rows.items()) +
                  f" kernels' share of the device sampler {share:.0f}%; host / device "
                  f"{rows['host twin'][0] / rows['device sampler'][0]:.1f}x; same clicks {same}")


if __name__ == "__main__":
    main()
