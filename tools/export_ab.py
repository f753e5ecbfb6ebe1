"""Per-frame export of the video predictor's masks for predict.json: the reference's host loop against the
device export (csrc/rle.hip), in one process, at the evaluation's 13 objects in 4 categories, smooth random
low-res logits at 128^2, exported to 1024 x 1280 and to 512 x 512.

  python tools/export_ab.py [--n 13] [--ncat 4] [--low 128] [--sizes 1024x1280 512x512] [--frames 8]
                            [--reps 5] [--rounds 3]

Host path (what the parent of this tool's commit had; reference eval/inference.py:487-514 + :870-901): the
[N, H, W] fp32 logits (ops.bilinear), per object `(logits[i] > 0).cpu().numpy()` and
`sigmoid(logits[i]).mean().item()`, np.logical_or per category, rle.encode and mask_to_bbox on the host.
Device path: s2h_mask_export + s2h_rle_transitions, one copy of header + scores + run boundaries to pinned
memory, rle.from_transitions (predictor.MergedFrame); timed serially (every frame waited for before the next
is enqueued) and with one frame in flight, as eval/inference.predict_on_video drives it.

Both paths are timed with a host clock around whole frames that end with the result on the host, alternated
over `rounds`; the results of the two paths are compared (strings, boxes, areas exactly, scores to 1e-5)
before anything is timed.  Prints one JSON line per size: ms per frame and bytes copied per frame."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sam2-video-training_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def field(N, S, seed):
    """smooth logits (white noise blurred twice with a 15 x 15 box, unit variance times 4, minus 1): a few
    blobs per object, as a tracked frame's masks"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, 1, S, S, generator=g)
    for _ in range(2):
        x = torch.nn.functional.avg_pool2d(x, 15, stride=1, padding=7)
    return (x[:, 0] / x.std() * 4.0 - 1.0).contiguous()


def host_frame(ops, rle, mask_to_bbox, low, H, W, cats):
    """the reference's loop -> (result in MergedFrame.result()'s layout, bytes copied)"""
    logits = ops.bilinear(low, H, W)
    masks, scores, nbytes = [], [], 0
    for i in range(low.shape[0]):
        m = (logits[i] > 0.0).cpu().numpy()
        scores.append(torch.sigmoid(logits[i]).mean().item())
        masks.append(m)
        nbytes += m.nbytes + 4
    out = {}
    for c, objs in enumerate(cats):
        merged = np.logical_or.reduce([masks[o] for o in objs], axis=0)
        if merged.sum() == 0:
            continue
        out[c] = {"segmentation": rle.encode(merged), "bbox": mask_to_bbox(merged), "area": int(merged.sum())}
    return {"categories": out, "scores": dict(enumerate(scores))}, nbytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=13)
    ap.add_argument("--ncat", type=int, default=4)
    ap.add_argument("--low", type=int, default=128)
    ap.add_argument("--sizes", nargs="+", default=["1024x1280", "512x512"])
    ap.add_argument("--frames", type=int, default=8, help="different frames cycled through")
    ap.add_argument("--reps", type=int, default=5, help="passes over the frames per timed window")
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("export_ab needs the GPU: there is no CPU timing of a device path")
    from sam2_video.data import rle
    from sam2_video.eval.utils import mask_to_bbox
    from sam2_video.kernels import ops
    from sam2_video.predictor import MergedFrame, StagingPool

    N, ncat = args.n, args.ncat
    cats = [[o for o in range(N) if o % ncat == c] for c in range(ncat)]
    off = torch.tensor(np.cumsum([0] + [len(c) for c in cats]), dtype=torch.int32).cuda()
    obj = torch.tensor([o for c in cats for o in c], dtype=torch.int32).cuda()
    frames = [field(N, args.low, 100 + k).cuda() for k in range(args.frames)]

    pool = StagingPool()  # one for the run, as an inference state keeps one for its clip

    def device_frame(low, H, W):
        return MergedFrame(low, H, W, list(range(N)), list(range(ncat)), off, obj, pool=pool)

    for size in args.sizes:
        H, W = (int(v) for v in size.lower().split("x"))
        n_trans = []
        for low in frames:  # the two paths agree (this is also the warm-up of both)
            want, host_bytes = host_frame(ops, rle, mask_to_bbox, low, H, W, cats)
            mf = device_frame(low, H, W)
            got = mf.result()
            assert list(got["categories"]) == list(want["categories"])
            for c in want["categories"]:
                assert got["categories"][c] == want["categories"][c], f"category {c} differs"
            assert max(abs(got["scores"][i] - want["scores"][i]) for i in range(N)) <= 1e-5
            n_trans.append(sum(len(rle.counts_from_string(v["segmentation"]["counts"])) for v in want["categories"].values()))
            dev_bytes = mf.bytes_copied
        torch.cuda.synchronize()

        host_ms, serial_ms, flight_ms = [], [], []
        count = args.reps * len(frames)
        for _ in range(args.rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.reps):
                for low in frames:
                    host_frame(ops, rle, mask_to_bbox, low, H, W, cats)
            host_ms.append((time.perf_counter() - t0) * 1e3 / count)

            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.reps):
                for low in frames:
                    device_frame(low, H, W).result()
            serial_ms.append((time.perf_counter() - t0) * 1e3 / count)

            torch.cuda.synchronize()
            t0 = time.perf_counter()
            prev = None
            for _ in range(args.reps):
                for low in frames:
                    cur = device_frame(low, H, W)
                    if prev is not None:
                        prev.result()
                    prev = cur
            prev.result()
            flight_ms.append((time.perf_counter() - t0) * 1e3 / count)

        # the device work alone (kernels + copy), by events, without the host decoding
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        keep = []
        a.record()
        for _ in range(args.reps):
            for low in frames:
                keep.append(device_frame(low, H, W))
        b.record()
        torch.cuda.synchronize()
        res = {"n": N, "ncat": ncat, "low": args.low, "H": H, "W": W, "frames_per_window": count,
               "runs_per_frame_mean": round(float(np.mean(n_trans)), 1),
               "host_ms_per_frame": [round(v, 3) for v in host_ms],
               "device_serial_ms_per_frame": [round(v, 3) for v in serial_ms],
               "device_one_in_flight_ms_per_frame": [round(v, 3) for v in flight_ms],
               "device_stream_ms_per_frame": round(a.elapsed_time(b) / count, 4),
               "host_bytes_per_frame": host_bytes, "device_bytes_per_frame": dev_bytes,
               "host_over_device_serial": round(min(host_ms) / min(serial_ms), 1),
               "host_over_device_one_in_flight": round(min(host_ms) / min(flight_ms), 1)}
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
