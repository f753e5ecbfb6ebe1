"""TEST INFRASTRUCTURE ONLY -- generates tests/golden/multimask/mm_tiny256_{point,box}.pt from the REFERENCE
itself in eval mode with the three-mask SAM heads on (imported through oracle/ref_harness.py; runs
only where the reference checkout exists).

The reference model is built by the harness from this build's config table, patched here with what
upstream's released configs and `build_sam2_video_predictor` set: multimask_output_in_sam,
multimask_output_for_tracking, use_multimask_token_for_obj_ptr, multimask_min_pt_num 0,
multimask_max_pt_num 1 and the decoder's dynamic_multimask_via_stability (delta 0.05, thresh 0.98
unless the search below moves it).  It runs forward_image -> prepare_prompt_inputs ->
forward_tracking under no_grad on a deterministic synthetic clip (Hiera-T, 256^2, 3 frames, 3
objects) with deterministic synthetic weights.

  mm_tiny256_point  one click per object: every frame takes the multimask path
  mm_tiny256_box    a box (two points): frame 0 takes the dynamic-stability path, frames 1.. multimask

Stored per frame t (plain tensors): low-res logits of the chosen mask [O, 1, 64, 64] (gated), the
three candidate IoUs [O, 3], token 0's IoU [O], the chosen token index [O], the object score [O, 1],
the object pointer [O, 256], token 0's stability score and its two areas [O], the path taken, and
the delta / threshold used.

A fixture is written only if the reference alone satisfies (asserted, margins printed):
  (a) every top-2 gap of the candidate IoUs is >= 1e-2 (ten times the 1e-3 logit tolerance of the
      parity tests), so the argmax cannot flip within tolerance;
  (b) for every object on the dynamic path the stable / unstable decision is the same when every
      pixel with | |logit| - delta | < 2e-3 is moved to either side of its threshold;
  (c) the box fixture has at least one stable and one unstable object on frame 0.
With upstream's 0.98 all objects of the synthetic weights are unstable, so for (c) the generator
searches clip index and weight seed and, where needed, puts the threshold halfway between two
observed stability scores, subject to (b).  What it chose is stored in the fixture; the test builds
its model from those values.

Usage:  python tools/gen_multimask_golden.py [mm_tiny256_point] [mm_tiny256_box]
"""
from __future__ import annotations

import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_harness as H  # noqa: E402
from gen_golden import reference_batch  # noqa: E402

# a directory of its own: tests/golden/*.pt is the closed set of training-step fixtures (tests/test_host.py)
OUT = os.path.join(ROOT, "tests", "golden", "multimask")
ALL = ["image_encoder", "memory_attention", "memory_encoder", "mask_decoder", "prompt_encoder"]
SHAPE = dict(size="tiny", image_size=256, T=3, n_cat=5, n_obj=3)
DELTA, UPSTREAM_THRESH = 0.05, 0.98
IOU_GAP, NEAR = 1e-2, 2e-3
FLAGS = {"multimask_output_in_sam": True, "multimask_output_for_tracking": True,
         "use_multimask_token_for_obj_ptr": True, "multimask_min_pt_num": 0, "multimask_max_pt_num": 1}


def _patched_config(thresh):
    """the config table the harness reads (model/configs.py model_config), with the multimask flags"""
    cfgmod = H.product_file("model/configs.py")
    orig = getattr(cfgmod, "_mm_orig_model_config", None) or cfgmod.model_config
    cfgmod._mm_orig_model_config = orig

    def model_config(size="tiny", image_size=512):
        cfg = orig(size, image_size)
        cfg.update(FLAGS)
        cfg["sam_mask_decoder_extra_args"] = {"dynamic_multimask_via_stability": True,
                                              "dynamic_multimask_stability_delta": DELTA,
                                              "dynamic_multimask_stability_thresh": float(thresh)}
        return cfg
    cfgmod.model_config = model_config


def run_reference(prompt, clip_idx, seed, thresh):
    """-> per-frame records of the reference's SAM heads in eval mode"""
    _patched_config(thresh)
    torch.manual_seed(0)
    model = H.build_reference_model(SHAPE["size"], SHAPE["image_size"], ALL, prompt, seed=seed)
    model.eval()
    dec = model.sam_mask_decoder
    assert dec.dynamic_multimask_via_stability and model.multimask_output_in_sam
    synth = H.product_file("data/synthetic.py")
    clip = synth.make_clip(clip_idx, SHAPE["T"], SHAPE["image_size"], SHAPE["n_cat"], SHAPE["n_obj"], None)
    batch = reference_batch(clip)
    frames, raw = [], {}
    heads, predict = model._forward_sam_heads, dec.predict_masks

    def predict_masks(*a, **k):
        out = predict(*a, **k)
        raw["masks"], raw["iou"] = out[0].detach().float(), out[1].detach().float()
        return out

    def forward_sam_heads(*a, **k):
        out = heads(*a, **k)
        frames.append({"multimask": bool(k.get("multimask_output", False)), "all_masks": raw["masks"],
                       "all_ious": raw["iou"], "ious": out[2].detach().float(), "low_res": out[3].detach().float(),
                       "obj_ptr": out[5].detach().float(), "obj_score": out[6].detach().float()})
        return out
    dec.predict_masks = predict_masks
    model._forward_sam_heads = forward_sam_heads
    with torch.no_grad():
        bo = model.forward_image(batch.flat_img_batch)
        bo = model.prepare_prompt_inputs(bo, batch)
        model.forward_tracking(bo, batch)
    assert len(frames) == SHAPE["T"]
    for fr in frames:
        m0 = fr["all_masks"][:, 0].flatten(1)
        fr["area_i"] = (m0 > DELTA).sum(-1)
        fr["area_u"] = (m0 > -DELTA).sum(-1)
        fr["stability"] = dec._get_stability_scores(fr["all_masks"][:, 0:1]).reshape(-1)
        best = 1 + fr["all_ious"][:, 1:].argmax(-1)
        stable = fr["stability"] >= thresh
        fr["best_idx"] = best if fr["multimask"] else torch.where(stable, torch.zeros_like(best), best)
        # (b): the range of the score when the pixels within NEAR of +-delta change side
        near_i_in = ((m0 > DELTA) & ((m0 - DELTA).abs() < NEAR)).sum(-1)
        near_i_out = ((m0 <= DELTA) & ((m0 - DELTA).abs() < NEAR)).sum(-1)
        near_u_in = ((m0 > -DELTA) & ((m0 + DELTA).abs() < NEAR)).sum(-1)
        near_u_out = ((m0 <= -DELTA) & ((m0 + DELTA).abs() < NEAR)).sum(-1)
        ai, au = fr["area_i"].float(), fr["area_u"].float()
        fr["stab_lo"] = torch.where(au + near_u_out > 0, (ai - near_i_in) / (au + near_u_out).clamp(min=1), ai * 0 + 1)
        fr["stab_hi"] = torch.where(au - near_u_in > 0, (ai + near_i_out) / (au - near_u_in).clamp(min=1), ai * 0 + 1)
    return model, clip, bo, frames


def iou_gap(frames):
    top2 = torch.cat([fr["all_ious"][:, 1:] for fr in frames]).topk(2, dim=-1).values
    return float((top2[:, 0] - top2[:, 1]).min())


def robust(fr, thresh):
    """(b) for a dynamic-path frame: both ends of every object's score range on one side of thresh"""
    return bool((((fr["stab_lo"] >= thresh) & (fr["stab_hi"] >= thresh))
                 | ((fr["stab_lo"] < thresh) & (fr["stab_hi"] < thresh))).all())


def search_box():
    """(clip_idx, seed, thresh) whose frame 0 has a stable and an unstable object, robustly"""
    for seed in range(0, 4):
        for clip_idx in range(7, 15):
            _, _, _, frames = run_reference("box", clip_idx, seed, UPSTREAM_THRESH)
            f0 = frames[0]
            assert not f0["multimask"]
            cands = [UPSTREAM_THRESH]
            sc = sorted(set(float(x) for x in f0["stability"]))
            cands += [0.5 * (a + b) for a, b in zip(sc, sc[1:])]
            for th in cands:
                stable = f0["stability"] >= th
                if bool(stable.any()) and not bool(stable.all()) and robust(f0, th):
                    print(f"box: clip {clip_idx} seed {seed}: frame-0 stability {[round(x, 5) for x in sc]} -> "
                          f"thresh {th:.6f}")
                    return clip_idx, seed, th
            print(f"box: clip {clip_idx} seed {seed}: stability {[round(x, 5) for x in sc]}: no robust split")
    raise SystemExit("no (clip, seed, thresh) gives a stable and an unstable object on frame 0")


def write_fixture(name, prompt, clip_idx, seed, thresh):
    model, clip, bo, frames = run_reference(prompt, clip_idx, seed, thresh)
    # the conditions the reference alone must satisfy
    gap = iou_gap(frames)
    assert gap >= IOU_GAP, f"{name}: (a) top-2 candidate IoU gap {gap:.4f} < {IOU_GAP}"
    dyn = [t for t, fr in enumerate(frames) if not fr["multimask"]]
    if prompt == "point":
        assert dyn == [], f"{name}: every frame must take the multimask path, dynamic frames {dyn}"
    else:
        assert dyn == [0], f"{name}: frame 0 dynamic, later frames multimask; got dynamic frames {dyn}"
        f0 = frames[0]
        assert robust(f0, thresh), f"{name}: (b) a stability decision can flip within {NEAR} of +-delta"
        stable = f0["stability"] >= thresh
        assert bool(stable.any()) and not bool(stable.all()), f"{name}: (c) stable {stable.tolist()}"
        margin = float(torch.minimum((f0["stab_lo"] - thresh).abs(), (f0["stab_hi"] - thresh).abs()).min())
        print(f"{name}: (b) score ranges {[(round(float(a), 5), round(float(b), 5)) for a, b in zip(f0['stab_lo'], f0['stab_hi'])]}"
              f" vs thresh {thresh:.6f}: worst margin {margin:.5f}; (c) stable {stable.tolist()}")
    print(f"{name}: (a) smallest top-2 candidate IoU gap {gap:.4f}; chosen "
          f"{[fr['best_idx'].tolist() for fr in frames]}")
    g = {"meta/T": torch.tensor(SHAPE["T"]), "meta/image_size": torch.tensor(SHAPE["image_size"]),
         "meta/seed": torch.tensor(seed), "meta/clip_idx": torch.tensor(clip_idx),
         "meta/parts": torch.tensor([], dtype=torch.long), "meta/prompt": prompt, "meta/size": SHAPE["size"],
         "meta/delta": torch.tensor(DELTA, dtype=torch.float64),
         "meta/thresh": torch.tensor(float(thresh), dtype=torch.float64),
         "in/images_sum": clip["images"].double().sum(), "in/masks_count": clip["masks"].sum(dim=(2, 3)),
         "obj_to_cat": torch.tensor(bo["obj_to_cat"])}
    pin = bo["point_inputs_per_frame"][0]
    g["prompt/coords"] = pin["point_coords"].detach().clone()
    g["prompt/labels"] = pin["point_labels"].detach().clone()
    for t, fr in enumerate(frames):
        g[f"obj/{t}/multimask"] = torch.tensor(int(fr["multimask"]))
        g[f"obj/{t}/low_res"] = fr["low_res"].clone()
        g[f"obj/{t}/cand_ious"] = fr["all_ious"][:, 1:].clone()
        g[f"obj/{t}/iou0"] = fr["all_ious"][:, 0].clone()
        g[f"obj/{t}/ious_out"] = fr["ious"].clone()
        g[f"obj/{t}/best_idx"] = fr["best_idx"].to(torch.int32)
        g[f"obj/{t}/obj_score"] = fr["obj_score"].clone()
        g[f"obj/{t}/obj_ptr"] = fr["obj_ptr"].clone()
        g[f"obj/{t}/stability"] = fr["stability"].clone()
        g[f"obj/{t}/area_i"] = fr["area_i"].to(torch.int32)
        g[f"obj/{t}/area_u"] = fr["area_u"].to(torch.int32)
        # consistency of the record with what the reference returned
        bi = torch.arange(fr["low_res"].shape[0])
        sel = fr["all_masks"][bi, fr["best_idx"]]
        gate = (fr["obj_score"] > 0).reshape(-1, 1, 1)
        assert torch.equal(torch.where(gate, sel, torch.full_like(sel, -1024.0)), fr["low_res"][:, 0])
    path = os.path.join(OUT, f"{name}.pt")
    torch.save(g, path)
    print(f"{name}: clip {clip_idx} seed {seed} thresh {thresh:.6f} -> {path} ({os.path.getsize(path) / 1e3:.0f} kB)")


def main(argv):
    os.makedirs(OUT, exist_ok=True)
    names = argv or ["mm_tiny256_point", "mm_tiny256_box"]
    if "mm_tiny256_point" in names:
        write_fixture("mm_tiny256_point", "point", 7, 0, UPSTREAM_THRESH)
    if "mm_tiny256_box" in names:
        write_fixture("mm_tiny256_box", "box", *search_box())


if __name__ == "__main__":
    main(sys.argv[1:])
