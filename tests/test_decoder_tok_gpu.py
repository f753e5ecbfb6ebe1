"""The two-way transformer's token side as fused launches (csrc/decoder_tok.hip, frametape.dec_self /
dec_post / dec_final) against its separate launches (S2H_DEC_TOK=0) on a bf16 training step.
The kernel-level float64 pins of every stored stage are in test_decoder_tok_kernels_gpu.py; the step-level
tests here stay as they are."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _close(a, b, tol):
    a = a.float()
    b = b.float()
    err = (a - b).abs().max().item()
    scale = b.abs().max().item() + 1e-6
    assert err <= tol * scale, f"max err {err:.3e} vs scale {scale:.3e} (tol {tol})"


@pytest.mark.parametrize("golden", ["bplus256_point_all", "bplus256_point_all_t8"])
def test_decoder_token_side_fused_matches_unfused_bf16(golden, monkeypatch):
    """a bf16 B+ 256^2 training step (the reference's fixture clip) with the decoder's token side fused
    (default) and unfused: the fused launches ran on every tracked frame's mask decoder, the per-stage
    mask logits and the loss agree to bf16 rounding, every mask-decoder weight gradient to cosine >= 0.98 and
    the whole gradient arena to >= 0.999 (the same ops in both, only fp32 summation order differs)"""
    from step_harness import build_model, golden_batch, grads_by_name, load_golden, mask_iou, run_step

    from sam2_video.kernels import frametape
    g = load_golden(golden)
    batch = golden_batch(g).to(DEV)
    calls = {"self": 0, "post": 0, "final": 0}
    orig = (frametape.dec_self, frametape.dec_post, frametape.dec_final)

    def count(name, fn):
        def f(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        return f
    monkeypatch.setattr(frametape, "dec_self", count("self", orig[0]))
    monkeypatch.setattr(frametape, "dec_post", count("post", orig[1]))
    monkeypatch.setattr(frametape, "dec_final", count("final", orig[2]))
    res = {}
    for flag in ("0", "1"):
        monkeypatch.setenv("S2H_DEC_TOK", flag)
        model = build_model("base_plus", 256, ["image_encoder", "memory_attention", "memory_encoder", "mask_decoder",
                                               "prompt_encoder"], "point", dtype="bf16")
        stages, merged, losses, _ = run_step(model, batch)
        res[flag] = ([s["pred_masks"].detach().float().cpu() for s in stages], float(losses["total_loss"]),
                     grads_by_name(model))
    assert calls["self"] > 0 and calls["post"] == calls["self"] and calls["final"] * 2 == calls["self"], calls
    (m0, l0, g0), (m1, l1, g1) = res["0"], res["1"]
    for a, b in zip(m0, m1):
        assert mask_iou(a, b) >= 0.99
        _close(a, b, 0.03)
    assert abs(l0 - l1) <= 3e-3 * abs(l0), (l0, l1)
    # key biases: zero gradient in exact arithmetic (softmax is shift-invariant along the keys); query
    # biases: a sum over every query row of a softmax gradient (the image -> token one over 1024 rows per
    # object) that nearly cancels -- both are rounding noise here, kept in the arena-wide cosine below
    dec = [n for n in g0 if "sam_mask_decoder.transformer." in n and g0[n].abs().max() > 0
           and not n.endswith(("k_proj.bias", "q_proj.bias"))]
    assert len(dec) > 50
    for n in dec:
        cos = torch.nn.functional.cosine_similarity(g0[n].flatten().double(), g1[n].flatten().double(), dim=0).item()
        # the same ops in bf16, fp32 summation order different (the fused kernels' MFMA order vs the
        # separate kernels' tiles): a bf16 rounding flips here and there and propagates through the image ->
        # token attention (a round-5 variant with the MLP's K split in two reached 1 - cos = 0.01 on its
        # projections' weight gradients); the bound against the reference itself is
        # test_training_step_gpu.py's bf16 gradient report (the reference's bf16-vs-fp32 drift)
        assert cos >= 0.98, (n, cos)
    flat0 = torch.cat([v.flatten() for v in g0.values()]).double()
    flat1 = torch.cat([v.flatten() for v in g1.values()]).double()
    assert torch.nn.functional.cosine_similarity(flat0, flat1, dim=0).item() >= 0.999


def test_decoder_token_kernels_weight_prefetch_bit_identical():
    """the token-side kernels with each projection's weight fragments issued a phase ahead (round 6,
    s2h_dec_sched(1), default) against each projection loading its own (0): the same MFMAs in the same
    order, so the whole bf16 training step -- masks, loss, every gradient -- is bit-identical"""
    from step_harness import build_model, golden_batch, grads_by_name, load_golden, run_step

    from sam2_video.kernels._lib import lib
    g = load_golden("bplus256_point_all")
    batch = golden_batch(g).to(DEV)
    res = {}
    prev = lib().s2h_dec_sched(-1)
    try:
        for mode in (0, 1):
            lib().s2h_dec_sched(mode)
            model = build_model("base_plus", 256, ["image_encoder", "memory_attention", "memory_encoder",
                                                   "mask_decoder", "prompt_encoder"], "point", dtype="bf16")
            stages, _, losses, _ = run_step(model, batch)
            torch.cuda.synchronize()
            res[mode] = ([s["pred_masks"].detach().float().cpu() for s in stages], float(losses["total_loss"]),
                         grads_by_name(model))
    finally:
        lib().s2h_dec_sched(prev)
    (m0, l0, g0), (m1, l1, g1) = res[0], res[1]
    assert l0 == l1
    for a, b in zip(m0, m1):
        assert torch.equal(a, b)
    assert g0.keys() == g1.keys()
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n
