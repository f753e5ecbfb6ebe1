"""Measurement of the training visualisation at the bench shape (B+ 512^2, 8 frames, 13 categories,
max_length 4), one process (profiles/viz_ab.log):

  1. the compositor's device time from HIP events: viz_pack of the ground truth and of the logits and viz_compose
     on tensors of the step's shapes, median of --reps after a warm-up;
  2. the wall time of a visualised step against the plain steps around it in the same run of the captured step
     graph (StepRunner, train_every_n_steps = --every), the visualised step split into the device stage, the copy
     back and Pillow's GIF encode.

    python tools/viz_ab.py [--steps 12] [--every 5] [--reps 20] [--out DIR]
"""
import argparse
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "sam2-video-training_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402


def kernel_time(reps, S=512, T=4, C=13):
    from sam2_video.kernels import ops
    from sam2_video.utils.viz import category_palette
    g = torch.Generator(device="cuda").manual_seed(0)
    frames = torch.randn(T, 3, S, S, device="cuda", generator=g)
    gt = torch.rand(T, C, S, S, device="cuda", generator=g) < 0.2
    logits = torch.randn(T, C, S, S, device="cuda", generator=g) * 4
    pal = torch.from_numpy(category_palette(C)).cuda()
    markers = torch.tensor([[0, 40 * i + 20, 30 * i + 25, 0, 0, 200, 40, 40] for i in range(C)], dtype=torch.int32).cuda()
    gw, pw = ops.viz_pack(gt), ops.viz_pack(logits)
    out = ops.viz_compose(frames, frames[0], gw, pw, pal, markers)
    rows = {"pack_gt": [], "pack_logits": [], "compose": [], "all": []}
    for r in range(reps + 3):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        ops.viz_pack(gt, out=gw)
        ev[1].record()
        ops.viz_pack(logits, out=pw)
        ev[2].record()
        ops.viz_compose(frames, frames[0], gw, pw, pal, markers, out=out)
        ev[3].record()
        torch.cuda.synchronize()
        if r >= 3:
            for k, (a, b) in zip(rows, ((0, 1), (1, 2), (2, 3), (0, 3))):
                rows[k].append(ev[a].elapsed_time(ev[b]))
    traffic = frames.numel() * 4 * 3 + gt.numel() + logits.numel() * 4 + 2 * (gw.numel() * 8) * 2 + out.numel()
    for k, v in rows.items():
        print(f"kernel {k:12s} median {statistics.median(v) * 1e3:8.1f} us  min {min(v) * 1e3:8.1f} us  ({len(v)} reps)")
    print(f"kernel bytes moved at least {traffic / 1e6:.1f} MB -> {traffic / statistics.median(rows['all']) / 1e6:.0f} GB/s "
          f"over the three launches; output {out.numel() / 1e6:.1f} MB")


def step_times(steps, every, out_dir):
    from sam2_video.data.synthetic import make_clip, sam2_collate_fn
    from sam2_video.kernels import functional as FN
    from sam2_video.model.sam2model import SAM2Model
    from sam2_video.training.trainer import SAM2LightningModule, StepRunner
    from sam2_video.utils import viz as V
    device = torch.device("cuda", 0)
    FN.set_seed(1234)
    all_mods = ["image_encoder", "memory_attention", "memory_encoder", "mask_decoder", "prompt_encoder"]
    model = SAM2Model(None, "base_plus@512", trainable_modules=all_mods, compute_dtype="bf16")
    loss_cfg = {"type": "multi_step", "weight_dict": {"loss_mask": 20, "loss_dice": 1, "loss_iou": 1, "loss_class": 0},
                "supervise_all_iou": True, "iou_use_l1_loss": True}
    opt_cfg = {"type": "AdamW", "lr": 4e-6, "weight_decay": 0.01, "betas": [0.9, 0.999], "warmup_factor": 0.15}
    viz = {"enabled": True, "train_every_n_steps": every, "val_first_batch_every_n_epochs": 0, "max_length": 4, "stride": 1,
           "caption": "viz_ab", "save_dir": out_dir}
    module = SAM2LightningModule(model, loss_cfg, opt_cfg, {"enabled": True, "num_cycles": 0.5}, viz)
    module.setup("fit", device)
    runner = StepRunner(module, total_steps=steps, graph=True)
    batches = [sam2_collate_fn([make_clip(i, 8, 512, 13, 13)]).to(device) for i in range(steps)]
    parts = {}
    make, save = V.create_visualization_gif, V.save_visualization

    def timed_make(*a, **kw):  # device stage (to a device tensor), then the copy back, timed apart
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        make(*a, **dict(kw, to_host=False))
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        host = make(*a, **kw)
        t2 = time.perf_counter()
        parts["device_ms"], parts["device_plus_copy_ms"] = (t1 - t0) * 1e3, (t2 - t1) * 1e3
        return host

    def timed_save(*a, **kw):
        t0 = time.perf_counter()
        r = save(*a, **kw)
        parts["encode_ms"] = (time.perf_counter() - t0) * 1e3
        parts["bytes"] = sum(os.path.getsize(f) for f in r)
        return r
    import sam2_video.utils as U
    U.create_visualization_gif, U.save_visualization = timed_make, timed_save
    plain = []
    for k in range(steps):
        parts.clear()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        runner(batches[k])
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        fired = "encode_ms" in parts
        if k >= 2 and not fired:
            plain.append(ms)
        note = ""
        if fired:
            note = (f"  VISUALISED: device stage {parts['device_ms']:.2f} ms, device stage again + copy back "
                    f"{parts['device_plus_copy_ms']:.2f} ms, Pillow GIF encode {parts['encode_ms']:.1f} ms "
                    f"({parts['bytes'] / 1e6:.2f} MB file); the timing wrapper runs the device stage twice")
        print(f"step {k + 1:3d} wall {ms:9.2f} ms{note}")
    print(f"plain steps (from the third on): median {statistics.median(plain):.2f} ms, min {min(plain):.2f}, "
          f"max {max(plain):.2f}; files: {sorted(os.listdir(out_dir))}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--every", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    print(f"device {torch.cuda.get_device_name(0)}; torch {torch.__version__}")
    kernel_time(args.reps)
    out = args.out or tempfile.mkdtemp(prefix="viz_ab_")
    step_times(args.steps, args.every, out)


if __name__ == "__main__":
    main()
