"""Hole filling of the predictor's low-res logits: the HIP kernels (ops.fill_holes) against the host scipy
path (predictor._fill_holes_host: two blocking copies + 2 N scipy labellings), in one process, at the
predictor's batch of 13 objects and the 128^2 / 256^2 low-res sizes.

  python tools/cc_bench.py [--n 13] [--sizes 128 256] [--reps 2000] [--host-reps 10] [--rounds 3]

Device path: HIP events around `reps` back-to-back calls after a warm-up, eager and replayed from a
captured HIP graph.  Host path: a host clock around calls that end with the result back on the device
(the copy back synchronises), the two alternated over `rounds`.  The outputs of the two paths are
compared bit for bit at every size before anything is timed.  Prints one JSON line per size."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sam2-video-training_amd"))

import torch  # noqa: E402


def field(N, S, seed):
    """smooth logits (a 5 x 5 box blur of white noise): blobs with small holes and sprinkles"""
    g = torch.Generator().manual_seed(seed)
    return torch.nn.functional.avg_pool2d(torch.randn(N, 1, S, S, generator=g), 5, stride=1, padding=2).contiguous()


def events_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=13)
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--reps", type=int, default=2000)
    ap.add_argument("--host-reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--max-area", type=int, default=8)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cc_bench needs the GPU: there is no CPU timing of a device path")
    from sam2_video.kernels import ops
    from sam2_video.predictor import _fill_holes_host

    for S in args.sizes:
        x = field(args.n, S, S).cuda()
        out = torch.empty_like(x)
        dev = ops.fill_holes(x, args.max_area, out=out)
        host = _fill_holes_host(x, args.max_area)
        torch.cuda.synchronize()
        assert torch.equal(dev.view(torch.int32), host.view(torch.int32)), "device and host paths differ"
        changed = int((dev != x).sum().item())

        for _ in range(10):  # warm-up of both paths
            ops.fill_holes(x, args.max_area, out=out)
        _fill_holes_host(x, args.max_area)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            ops.fill_holes(x, args.max_area, out=out)
        g.replay()
        torch.cuda.synchronize()

        eager, graph, hostt = [], [], []
        for _ in range(args.rounds):
            eager.append(events_ms(lambda: ops.fill_holes(x, args.max_area, out=out), args.reps))
            graph.append(events_ms(g.replay, args.reps))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.host_reps):
                _fill_holes_host(x, args.max_area)
            torch.cuda.synchronize()
            hostt.append((time.perf_counter() - t0) * 1e3 / args.host_reps)
        res = {"n": args.n, "size": S, "max_area": args.max_area, "pixels_changed": changed,
               "device_eager_ms": [round(v, 4) for v in eager], "device_graph_ms": [round(v, 4) for v in graph],
               "host_ms": [round(v, 3) for v in hostt],
               "host_over_device_eager": round(min(hostt) / min(eager), 1),
               "host_over_device_graph": round(min(hostt) / min(graph), 1)}
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
