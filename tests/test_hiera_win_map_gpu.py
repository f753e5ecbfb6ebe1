"""Hiera's padded windows attended straight from the image layout (S2H_HIERA_WIN_MAP=1: the flash
kernels read q / k / v of the fused projection [B, H, W, 3 d] and write o / dqkv in place through a row
map, csrc/flash.hip s2h_flash_win_fwd, flash_bwd.hip s2h_flash_win_bwd) against the partitioned path
(=0: window_pad + the flash kernels on the [windows, 196, ...] copy + window_unpartition +
window_pad_colsum).  Both run the same arithmetic per query and per key, so every comparison is
torch.equal.

The mode is built for launches whose partitioned form runs without a key split (>= 256 batch-heads of
196 positions: the flagship step has 576); with fewer, the partitioned kernels sum fp32 key-split
partials in another order (measured: o differs by 1 bf16 ulp at 16 batch-heads), so the mode declines
and the block keeps the partitioned launches.  The kernel-level cases therefore use the smallest batch
that reaches 256 batch-heads; the same geometries at the small batch assert the fall-back."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _ops():
    from sam2_video.kernels import ops
    return ops


def _inputs(B, H, W, nh, hd, seed=0):
    gen = torch.Generator(DEV).manual_seed(seed)
    d = nh * hd
    qkv = torch.randn(B, H, W, 3 * d, device=DEV, generator=gen).to(torch.bfloat16)
    bias = torch.randn(3 * d, device=DEV, generator=gen) * 0.5
    do = torch.randn(B, H, W, d, device=DEV, generator=gen).to(torch.bfloat16)
    gb0 = torch.randn(3 * d, device=DEV, generator=gen)  # the bias gradient accumulates into this
    return qkv, bias, do, gb0


def _partitioned(qkv, bias, do, gb0, ws, nh):
    """the switch-0 launches: bias-row partition, attention on the windows, unpartition, column sums"""
    ops = _ops()
    B, H, W, d3 = qkv.shape
    d, hd, L = d3 // 3, d3 // 3 // nh, ws * ws
    scale = 1.0 / math.sqrt(hd)
    qkvw = ops.window_pad(qkv, ws, bias)
    nwin = qkvw.shape[0]
    q5 = qkvw.view(nwin, L, 3, nh, hd)
    q, k, v = q5[:, :, 0], q5[:, :, 1], q5[:, :, 2]
    ow = torch.empty(nwin, L, nh, hd, device=DEV, dtype=qkv.dtype)
    lse = torch.empty(nwin, nh, L, device=DEV, dtype=torch.float32)
    ops.attn_fwd(q, k, v, ow, lse, scale)
    o = ops.window_unpartition(ow.view(nwin, ws, ws, d), ws, B, H, W)
    dow = ops.window_partition(do, ws).view(nwin, L, nh, hd)
    dqkvw = torch.empty_like(q5)
    ops.attn_bwd(q, k, v, ow, dow, lse, dqkvw[:, :, 0], dqkvw[:, :, 1], dqkvw[:, :, 2], scale)
    gb = gb0.clone()
    ops.window_pad_colsum(dqkvw.view(nwin, ws, ws, d3), ws, B, H, W, gb)
    dqkv = ops.window_unpartition(dqkvw.view(nwin, ws, ws, d3), ws, B, H, W)
    return o, lse, dqkv, gb


def _mapped(qkv, bias, do, gb0, ws, nh, padrow=None):
    """the switch-1 launches"""
    ops = _ops()
    B, H, W, d3 = qkv.shape
    d, hd = d3 // 3, d3 // 3 // nh
    scale = 1.0 / math.sqrt(hd)
    assert ops.flash_win_ok(qkv, ws, nh)
    if padrow is None:
        padrow = ops.cast(bias, torch.bfloat16)
    o, lse = ops.flash_win_fwd(qkv, ws, nh, padrow, scale)
    dqkv, dpad = ops.flash_win_bwd(qkv, ws, nh, padrow, o, do, lse, scale)
    P = (-(-H // ws)) * ws * (-(-W // ws)) * ws - H * W
    gb = gb0.clone()
    ops.pad_rows_colsum(dpad, B, P, gb[d:])
    return o, lse, dqkv, gb, dpad


def _real_mask(B, H, W, ws, nh):
    """[B * nW, nh, L] bool: the window positions that hold a token"""
    row, _, _ = _ops().window_map_host(H, W, ws)
    m = torch.from_numpy(row >= 0).to(DEV)
    return m[None, :, None, :].expand(B, -1, nh, -1).reshape(B * m.shape[0], nh, m.shape[1])


@pytest.mark.parametrize("B,H,W,nh,hd", [(2, 16, 16, 2, 56), (1, 32, 32, 8, 56), (1, 20, 17, 2, 56), (1, 16, 16, 2, 72)])
def test_small_batches_decline_the_mode(B, H, W, nh, hd):
    """fewer than 256 batch-heads: the partitioned launches split their key range, the mode does not apply"""
    qkv, _, _, _ = _inputs(B, H, W, nh, hd)
    assert not _ops().flash_win_ok(qkv, 14, nh)


@pytest.mark.parametrize("B,H,W,nh,hd", [
    (32, 16, 16, 2, 56),  # full, right-partial, bottom-partial and corner windows (196 / 28 / 28 / 4 real rows)
    (4, 32, 32, 8, 56),   # the bench geometry: 3 x 3 windows, 8 heads
    (32, 20, 17, 2, 56),  # odd extents
    (32, 16, 16, 2, 72),  # the 128-wide image (Hiera-L's head dim)
])
def test_window_map_kernels_equal_the_partitioned_launches(B, H, W, nh, hd):
    ops = _ops()
    ops.wgrad_workspace(DEV)  # the fixed-order column sums' workspace
    ws = 14
    qkv, bias, do, gb0 = _inputs(B, H, W, nh, hd, seed=H * 100 + W + hd)
    o0, lse0, dqkv0, gb_ref = _partitioned(qkv, bias, do, gb0, ws, nh)
    o1, lse1, dqkv1, gb_new, _ = _mapped(qkv, bias, do, gb0, ws, nh)
    torch.cuda.synchronize()
    assert torch.equal(o1, o0)
    real = _real_mask(B, H, W, ws, nh)
    assert real.sum().item() == B * nh * H * W
    assert torch.equal(lse1.view(lse0.shape)[real], lse0[real])
    assert torch.isinf(lse1.view(lse0.shape)[~real]).all()
    assert torch.equal(dqkv1, dqkv0)
    assert torch.equal(gb_new, gb_ref)
    assert not torch.equal(gb_new, gb0)  # the padded keys' column sums did land


def test_window_map_comparison_can_fail():
    """the padded positions do reach the result: another bias row changes the real queries' outputs, and
    another dO of one real token changes the padded keys' gradients"""
    ops = _ops()
    ops.wgrad_workspace(DEV)
    B, H, W, nh, hd, ws = 32, 16, 16, 2, 56, 14
    qkv, bias, do, gb0 = _inputs(B, H, W, nh, hd, seed=5)
    o1, _, dqkv1, gb1, dpad1 = _mapped(qkv, bias, do, gb0, ws, nh)
    pr = ops.cast(bias, torch.bfloat16)
    pr2 = pr.clone()
    pr2[nh * hd:] += 1.0  # the k and v thirds of the bias row
    o2, _, _, _, _ = _mapped(qkv, bias, do, gb0, ws, nh, padrow=pr2)
    torch.cuda.synchronize()
    changed = (o1 != o2).any(-1)  # [B, H, W]
    assert changed[0, 15, 15] and changed[0, 0, 15] and changed[0, 15, 0]  # tokens of padded windows
    assert not changed[0, :14, :14].any()                                  # the full window has no padded key
    do2 = do.clone()
    do2[0, 15, 15] += 1.0  # the corner window: 4 real tokens, 192 padded keys
    _, _, dqkv2, gb2, dpad2 = _mapped(qkv, bias, do2, gb0, ws, nh)
    torch.cuda.synchronize()
    assert not torch.equal(dpad2, dpad1) and not torch.equal(gb2, gb1)
    assert torch.equal(dqkv2[0, :14, :14], dqkv1[0, :14, :14])


def _block(cd=torch.bfloat16, B=2):
    from sam2_video.kernels.arena import ParamArena
    from sam2_video.model.modeling.backbones.hieradet import MultiScaleBlock
    _ops().wgrad_workspace(DEV)
    torch.manual_seed(11)
    blk = MultiScaleBlock(448, 448, 8, window_size=14)
    for p in blk.parameters():
        p.data = torch.randn_like(p) * 0.05
    arena = ParamArena(list(blk.named_parameters()), [n for n, _ in blk.named_parameters()], cd, DEV)
    gen = torch.Generator(DEV).manual_seed(3)
    x0 = torch.randn(B, 32, 32, 448, device=DEV, generator=gen).to(cd)
    g = torch.randn(B, 32, 32, 448, device=DEV, generator=gen).to(cd)
    return blk, arena, x0, g


def _run_block(blk, arena, x0, g):
    arena.grad.zero_()
    x = x0.clone().requires_grad_(True)
    y = blk(x)
    y.backward(g)
    return y.detach(), x.grad


@pytest.mark.parametrize("B", [2, 4])
def test_padded_window_block_switch_0_equals_1(B, monkeypatch):
    """one stage-3 block of Hiera-B+ at 512^2 (32 x 32 tokens, window 14): output, input gradient and the
    whole gradient arena.  4 images (288 batch-heads) run the mode; 2 images (144) decline it"""
    from sam2_video.kernels import functional as FN
    blk, arena, x0, g = _block(B=B)
    calls = []
    real = FN.pad_window_attention
    monkeypatch.setattr(FN, "pad_window_attention", lambda *a, **k: calls.append(1) or real(*a, **k))
    res = {}
    for flag in ("0", "1"):
        monkeypatch.setenv("S2H_HIERA_WIN_MAP", flag)
        y, dx = _run_block(blk, arena, x0, g)
        torch.cuda.synchronize()
        res[flag] = (y.clone(), dx.clone(), arena.grad.clone())
    assert calls == ([1] if B == 4 else [])
    for a, b in zip(res["0"], res["1"]):
        assert torch.equal(a, b)
    assert res["1"][2].abs().sum().item() > 0


def test_fp32_compute_keeps_the_partitioned_path(monkeypatch):
    """outside the mode's domain the block falls back to today's launches (asserted, not assumed)"""
    from sam2_video.kernels import functional as FN
    blk, arena, x0, g = _block(torch.float32, B=4)
    calls = []
    real = FN.pad_window_attention
    monkeypatch.setattr(FN, "pad_window_attention", lambda *a, **k: calls.append(1) or real(*a, **k))
    monkeypatch.setenv("S2H_HIERA_WIN_MAP", "1")
    _run_block(blk, arena, x0, g)
    torch.cuda.synchronize()
    assert calls == []


def test_padded_window_block_capture_and_replay_equal_eager(monkeypatch):
    """forward + backward of the block captured into a graph (the row map, the zero row and the
    reduction workspace exist from the eager run) and replayed on new inputs equals the eager run"""
    monkeypatch.setenv("S2H_HIERA_WIN_MAP", "1")
    blk, arena, x0, g = _block(B=4)
    assert _ops().flash_win_ok(torch.empty(4, 32, 32, 3 * 448, device=DEV, dtype=torch.bfloat16), 14, 8)
    want = [t.clone() for t in _run_block(blk, arena, x0, g)] + [arena.grad.clone()]
    torch.cuda.synchronize()
    xs = torch.zeros_like(x0).requires_grad_(True)
    gs = torch.zeros_like(g)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up on the capture's side stream
        blk(xs).backward(gs)
    torch.cuda.current_stream().wait_stream(side)
    xs.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        arena.grad.zero_()
        ys = blk(xs)
        ys.backward(gs)
    with torch.no_grad():
        xs.copy_(x0)
        gs.copy_(g)
    arena.grad.fill_(7.0)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(ys.detach(), want[0])
    assert torch.equal(xs.grad, want[1])
    assert torch.equal(arena.grad, want[2])
