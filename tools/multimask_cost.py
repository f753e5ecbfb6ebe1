"""GPU kernel time of the three-mask SAM heads against the single-mask heads in the video predictor
(DESIGN.md §8 f3): the same 3-frame Hiera-T 256^2 clip, one click on each of 3 objects, propagated
PASSES times, under `rocprofv3 --kernel-trace`.

    rocprofv3 --kernel-trace -d OUT/on  -o kt -- python tools/multimask_cost.py --multimask 1
    rocprofv3 --kernel-trace -d OUT/off -o kt -- python tools/multimask_cost.py --multimask 0
    python tools/multimask_cost.py --diff OUT/off/kt_results.db OUT/on/kt_results.db

--diff prices every kernel name at (launches per pass) x (median duration), so the first pass's cold
launches do not count, and lists the names whose time per pass differs."""
import argparse
import collections
import glob
import os
import re
import sqlite3
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sam2-video-training_amd"))
PASSES, FRAMES, OBJECTS = 4, 3, 3


def run(multimask):
    import torch
    from sam2_video.data.synthetic import synthetic_batch
    from sam2_video.predictor import build_sam2_video_predictor
    pred = build_sam2_video_predictor("tiny", image_size=256, compute_dtype="bf16", multimask=bool(multimask),
                                      apply_postprocessing=False)
    clip = synthetic_batch(5, FRAMES, 256, 4, OBJECTS).img_batch[:, 0]
    pts = [[90.0, 120.0], [60.0, 60.0], [200.0, 180.0]]
    for _ in range(PASSES):
        st = pred.init_state(clip)
        for i, p in enumerate(pts):
            pred.add_new_points_or_box(st, 0, obj_id=i + 1, points=[p], labels=[1])
        n = sum(1 for _ in pred.propagate_in_video(st))
        assert n == FRAMES
    torch.cuda.synchronize()


def per_pass(db):
    path = db if os.path.isfile(db) else (glob.glob(os.path.join(db, "**", "*results.db"), recursive=True) or [db])[0]
    rows = sqlite3.connect(path).execute("select name, start, end from kernels").fetchall()
    by = collections.defaultdict(list)
    for n, s, e in rows:
        by[re.sub(r"\(.*", "", str(n))].append((e - s) / 1e3)
    out = {}
    for k, v in by.items():
        v.sort()
        out[k] = (len(v) / PASSES, v[len(v) // 2])
    return out


def diff(a, b):
    ka, kb = per_pass(a), per_pass(b)
    tot = lambda k: sum(n * m for n, m in k.values())  # noqa: E731
    ta, tb = tot(ka), tot(kb)
    print(f"kernel time per pass ({FRAMES} frames, {OBJECTS} objects): single-mask {ta:.1f} us, multimask {tb:.1f} us, "
          f"{tb - ta:+.1f} us ({100 * (tb - ta) / ta:+.2f} %); launches per pass {sum(n for n, _ in ka.values()):.0f} -> "
          f"{sum(n for n, _ in kb.values()):.0f}")
    names = sorted(set(ka) | set(kb), key=lambda n: -abs(kb.get(n, (0, 0))[0] * kb.get(n, (0, 0))[1]
                                                           - ka.get(n, (0, 0))[0] * ka.get(n, (0, 0))[1]))
    for n in names[:16]:
        (na, ma), (nb, mb) = ka.get(n, (0, 0.0)), kb.get(n, (0, 0.0))
        print(f"{nb * mb - na * ma:+9.1f} us  single {na:6.1f} x {ma:7.2f} us  multi {nb:6.1f} x {mb:7.2f} us  {n[:90]}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--multimask", type=int, default=1)
    ap.add_argument("--diff", nargs=2)
    x = ap.parse_args()
    if x.diff:
        diff(*x.diff)
    else:
        run(x.multimask)
