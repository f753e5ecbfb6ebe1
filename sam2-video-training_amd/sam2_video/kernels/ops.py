"""Tensor-level launchers for libsam2hip (no autograd).  Every function launches
on torch's current HIP stream and returns its output tensor(s).

Conventions: activations are float32 (fp32-parity mode) or bfloat16 (compute
mode); norms' gamma/beta, biases, LSE/statistics and weight gradients are fp32.
"""
from __future__ import annotations

import contextlib
import math
import os

import numpy as np
import torch

from ._lib import call, lib

F32, BF16 = 0, 1
ACT = {None: 0, "none": 0, "relu": 1, "gelu": 2, "sigmoid": 3}


def dt(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.bfloat16:
        return BF16
    raise TypeError(f"libsam2hip supports float32/bfloat16 activations, got {t.dtype}")


def ptr(t):
    return None if t is None else t.data_ptr()


def stream():
    return torch.cuda.current_stream().cuda_stream


_SIDE = {"on": os.environ.get("S2H_WGRAD_STREAM", "0") == "1", "streams": {}}


class SideWork:
    """Weight-gradient launches of one frame-tape backward on a second HIP stream, beside the
    input-gradient chain on the current one: a Linear's dW = dY^T X does not feed the next
    dgrad, so the two streams fill each other's ramp-up and tail (the step's GEMMs are short-K
    and latency-bound).  run(*reads) forks the side stream off the current one (an event) and
    keeps the tensors it reads alive; join() makes the current stream wait for everything
    forked and releases them -- the tape calls it before its gradients leave the backward, so
    nothing outside ever sees the second stream.  Graph capture records the fork / join as
    branches of the captured graph.  Opt-in (S2H_WGRAD_STREAM=1): on MI355X the second stream costs
    2.5 % of the bench step (59.5 vs 58.0 ms, profiles/r04_v4_wgrad_stream_ab.log) -- the weight
    gradients take CUs from the critical dgrad / attention-backward chain rather than filling idle
    ones (round 2 measured -4 % for the autograd form)."""

    def __init__(self):
        self.cur = self.ws = None
        _det_workspace_mode(not _SIDE["on"])
        if _SIDE["on"] and torch.cuda.is_available():
            self.cur = torch.cuda.current_stream()
            dev = self.cur.device
            ws = _SIDE["streams"].get(dev)
            if ws is None:
                ws = _SIDE["streams"][dev] = torch.cuda.Stream(dev)
            self.ws = ws
        self.refs = []
        self.used = False

    @contextlib.contextmanager
    def run(self, *reads):
        if self.ws is None:
            yield
            return
        self.ws.wait_stream(self.cur)
        with torch.cuda.stream(self.ws):
            yield
        self.refs.extend(t for t in reads if t is not None)
        self.used = True

    def join(self):
        if self.used:
            self.cur.wait_stream(self.ws)
        self.refs.clear()
        self.used = False


def _dev(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("libsam2hip kernels run on the GPU only (tensor on %s)" % t.device)


_RNG_OFFSET = {}


def rng_offset(device):
    """The device-resident uint64 dropout offset bound into libsam2hip (s2h_rng_bind): one per
    process, never freed (the library keeps its address).  Write it before a step (a fill
    kernel, no host sync) to draw fresh dropout masks, also on a replayed HIP graph."""
    t = _RNG_OFFSET.get("t")
    if t is None:
        t = torch.zeros(1, dtype=torch.int64, device=device)
        call("s2h_rng_bind", t.data_ptr())
        _RNG_OFFSET["t"] = t
    elif t.device.index != (torch.device(device).index if torch.device(device).index is not None
                            else torch.cuda.current_device()):
        raise RuntimeError(f"rng offset already bound on {t.device}, requested {device}")
    return t


# Workspace of the deterministic long-reduction weight-gradient GEMM (csrc/gemm_wgrad.hip): fp32
# partial tiles of <= ~256 (split, tile) workgroups x 256 KB plus the bias-gradient partials.  One per
# process, registered once, never freed (the library keeps its address); the GEMMs that use it are
# ordered on one stream -- with the opt-in weight-gradient side stream (S2H_WGRAD_STREAM) the library
# keeps the atomic split-K path instead (kmin 0).
WGRAD_WS_BYTES = 96 << 20
_WG_WS = {}


def _capturing():
    return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


def _persistent_alloc(what, n, dtype, device):
    """a buffer the library keeps the address of for the life of the process: never from a graph's
    private pool (a capture's allocations are released with the graph, the library would keep a
    dangling pointer) -- allocate it before the first capture (SAM2Model.load / StepRunner's eager
    warm-up do)"""
    if _capturing():
        raise RuntimeError(f"libsam2hip {what}: first use inside a HIP graph capture; allocate it before capturing "
                           f"(ops.{what}(device))")
    return torch.empty(n, dtype=dtype, device=device)


def _device_of(device):
    d = torch.device(device if device is not None else "cuda")
    if d.index is None:
        d = torch.device("cuda", torch.cuda.current_device())
    return d


WGRAD_KMIN = 4096  # csrc/gemm_wgrad.hip g_wg_kmin: reductions at least this long take the deterministic kernel


def _det_workspace_mode(on):
    """the library's deterministic-reduction workspace on (the default) or off: every user of it (the
    weight-gradient kernel, split-K partial tiles, fixed-order column sums) is ordered on ONE stream, so
    with the weight-gradient side stream (S2H_WGRAD_STREAM=1) they fall back to their atomic forms"""
    t = _WG_WS.get("t")
    if t is not None and _WG_WS.get("on", True) != on:
        call("s2h_wgrad_workspace", t.data_ptr(), WGRAD_WS_BYTES, WGRAD_KMIN if on else 0)
    _WG_WS["on"] = on


def wgrad_workspace(device=None):
    d = _device_of(device)
    t = _WG_WS.get("t")
    if t is None:
        t = _persistent_alloc("wgrad_workspace", WGRAD_WS_BYTES // 4, torch.float32, d)
        on = not _SIDE["on"]
        call("s2h_wgrad_workspace", t.data_ptr(), WGRAD_WS_BYTES, WGRAD_KMIN if on else 0)
        _WG_WS["t"] = t
        _WG_WS["on"] = on
    elif t.device != d:  # one registration per process: the library holds one address
        raise RuntimeError(f"wgrad workspace already registered on {t.device}, requested {d}")
    return t


# Deferred gradient sums (csrc/grad_defer.hip): inside the scope, the fixed-order second pass of the
# column reductions whose destination lies in `sink` (the gradient arena: LayerNorm gamma / beta, bias
# gradients) is recorded and run for all of them in a few launches when the scope closes.  The scope
# must enclose whole backward passes whose arena gradients nothing reads before it closes (the
# StepRunner's backward phases; the DDP all-reduce of a range is issued after its phase's scope).
# S2H_GRAD_DEFER=0 keeps the immediate second pass (A/B).
GRAD_DEFER_BYTES = 256 << 20
_DEFER = {"t": None, "depth": 0}


def grad_defer_enabled():
    return os.environ.get("S2H_GRAD_DEFER", "1") == "1"


@contextlib.contextmanager
def deferred_grad_sums(sink):
    if sink is None or not sink.is_cuda or _DEFER["depth"] > 0 or not grad_defer_enabled():
        _DEFER["depth"] += 1
        try:
            yield
        finally:
            _DEFER["depth"] -= 1
        return
    t = _DEFER["t"]
    if t is None or t.device != sink.device:
        t = _DEFER["t"] = _persistent_alloc("deferred_grad_sums", GRAD_DEFER_BYTES // 4, torch.float32, sink.device)
    call("s2h_grad_defer", t.data_ptr(), GRAD_DEFER_BYTES, sink.data_ptr(), sink.numel() * sink.element_size())
    _DEFER["depth"] += 1
    try:
        yield
    finally:
        _DEFER["depth"] -= 1
        try:
            call("s2h_grad_defer_flush", stream())
        finally:  # the scope ends even when the flush raised: later scopes must be able to register
            call("s2h_grad_defer_reset")


# ----------------------------------------------------------------- GEMM
def _operand_dtype(what, t, want):
    """the GEMM epilogues read the residual and the saved pre-activation as the A / B element type
    (bf16 for the MX-fp8 kernel) whatever the output type, and the column scale as fp32: a tensor of
    another type would be misread silently, so it is refused here"""
    if t is not None and t.dtype != want:
        raise TypeError(f"libsam2hip GEMM: {what} must be {want} (the kernel reads it as that type), got {t.dtype}")


def gemm(a, b, c, *, M, N, K, lda_m, lda_k, ldb_k, ldb_n, ldc, batch=1, sA=0, sB=0, sC=0,
         bias=None, bias_mode=1, residual=None, ldr=0, sR=0, aux=None, ldx=0, sX=0, aux_mode=0,
         cscale=None, drop_p=0.0, seed=0, alpha=1.0, beta=0.0, act=0, drop_idx0=0):
    _operand_dtype("residual", residual, a.dtype)
    _operand_dtype("aux", aux, a.dtype)
    _operand_dtype("cscale", cscale, torch.float32)
    _dev(a, b, c, bias, residual, aux, cscale)
    if bias is not None:
        assert bias.dtype == torch.float32 and bias.is_contiguous()
    if c.dtype == torch.float32 and K >= 512 and "t" not in _WG_WS:
        wgrad_workspace(c.device)
    call("s2h_gemm", dt(a), dt(c), batch, M, N, K,
         ptr(a), lda_m, lda_k, sA, ptr(b), ldb_k, ldb_n, sB, ptr(c), ldc, sC,
         ptr(bias), bias_mode, ptr(residual), ldr, sR, ptr(aux), ldx, sX, aux_mode,
         ptr(cscale), float(drop_p), int(seed) & (2**64 - 1), int(drop_idx0), float(alpha), float(beta), int(act),
         stream())
    return c


def _rows(x):
    assert x.stride(-1) == 1, "last dim must be contiguous"
    return x.numel() // x.shape[-1], x.shape[-1]


def linear(x, w, bias=None, act=None, out=None, pre=None, residual=None, out_dtype=None, cscale=None,
           drop_p=0.0, seed=0, drop_idx0=0):
    """out = drop(act(x @ w^T + bias) * cscale) (+ residual); optionally stores the pre-activation in `pre`."""
    x2 = x.reshape(-1, x.shape[-1])
    M, K = x2.shape
    N = w.shape[0]
    assert w.shape[1] == K and w.is_contiguous()
    if out is None:
        out = torch.empty(*x.shape[:-1], N, device=x.device, dtype=out_dtype or x.dtype)
    o2 = out.view(-1, N)
    r2 = residual.reshape(-1, N) if residual is not None else None
    p2 = pre.view(-1, N) if pre is not None else None
    gemm(x2, w, o2, M=M, N=N, K=K, lda_m=x2.stride(0), lda_k=1, ldb_k=1, ldb_n=K, ldc=N,
         bias=bias, residual=r2, ldr=N, aux=p2, ldx=N, aux_mode=1 if pre is not None else 0, act=ACT[act],
         cscale=cscale, drop_p=drop_p, seed=seed, drop_idx0=drop_idx0)
    return out


def rope_blocks(y2, rp, inverse=False):
    """in place axial RoPE of a [rows, N] matrix (C contiguous): rp = (cos, sin, L, nrot, period,
    ncol, dh) rotates, in every block of L rows, the rows < nrot in the columns < ncol (dh-wide
    heads, pairs (2i, 2i + 1))"""
    cos, sin, L, nrot, period, ncol, dh = rp
    rows, N = y2.shape
    assert rows % L == 0 and y2.stride(1) == 1
    ld = y2.stride(0)
    for c0 in range(0, ncol, dh):
        v = torch.as_strided(y2, (rows // L, L, dh), (L * ld, ld, 1), y2.storage_offset() + c0)
        rope(v, v, nrot, cos, sin, period, inverse)
    return y2


def linear_rope(x, w, bias, rp, out=None):
    """out = RoPE(x @ w^T + bias) (rope_blocks' layout): one GEMM with the rotation in its epilogue
    in bf16 (s2h_linear_rope), GEMM + in-place rotation in fp32"""
    x2 = x.reshape(-1, x.shape[-1])
    M, K = x2.shape
    N = w.shape[0]
    assert w.shape[1] == K and w.is_contiguous()
    if out is None:
        out = torch.empty(*x.shape[:-1], N, device=x.device, dtype=x.dtype)
    o2 = out.view(-1, N)
    cos, sin, L, nrot, period, ncol, dh = rp
    if x.dtype == torch.bfloat16 and x2.stride(1) == 1:
        _dev(x2, w, o2, bias)
        call("s2h_linear_rope", M, N, K, ptr(x2), x2.stride(0), ptr(w), w.stride(0), ptr(bias), ptr(o2), N, ptr(cos),
             ptr(sin), int(L), int(nrot), int(period), int(ncol), int(dh), stream())
        return out
    linear(x, w, bias, out=out)
    rope_blocks(o2, rp)
    return out


def linear_add_ln(x, w, bias, residual, gamma, beta, eps, drop_p=0.0, seed=0, drop_idx0=0, xsum=None, y=None,
                  mean=None, rstd=None):
    """xsum = residual + dropout(x @ w^T + bias), y = LN(xsum) (gamma, beta, eps), mean / rstd per row, in
    one launch (s2h_linear_add_ln; bf16, N = 128 or 256); returns (y, xsum, mean, rstd)"""
    x2 = x.reshape(-1, x.shape[-1])
    M, K = x2.shape
    N = w.shape[0]
    assert w.shape[1] == K and w.is_contiguous() and x2.stride(1) == 1 and x.dtype == torch.bfloat16
    shape = (*x.shape[:-1], N)
    xsum = torch.empty(shape, device=x.device, dtype=x.dtype) if xsum is None else xsum
    y = torch.empty(shape, device=x.device, dtype=x.dtype) if y is None else y
    mean = torch.empty(M, device=x.device, dtype=torch.float32) if mean is None else mean
    rstd = torch.empty(M, device=x.device, dtype=torch.float32) if rstd is None else rstd
    r2 = residual.reshape(-1, N) if residual is not None else None
    _dev(x2, w, bias, r2, xsum, y, gamma, beta, mean, rstd)
    call("s2h_linear_add_ln", M, N, K, ptr(x2), x2.stride(0), ptr(w), w.stride(0), ptr(bias), ptr(r2),
         r2.stride(0) if r2 is not None else 0, float(drop_p), int(seed) & (2**64 - 1), int(drop_idx0), ptr(xsum), N,
         ptr(gamma), ptr(beta), float(eps), ptr(y), N, ptr(mean), ptr(rstd), stream())
    return y, xsum, mean, rstd


def linear_dgrad(dy, w, dx=None, accumulate=False, pre=None, act=None, alpha=1.0, residual=None):
    """dx = alpha * dy @ w   (optionally * act'(pre) elementwise, fusing the previous layer's
    activation grad; for ReLU `pre` may be the previous layer's output, and alpha its 1/keep);
    accumulate: dx += ...; residual [rows, K] (same dtype, contiguous): dx = ... + residual (one
    rounding of the fp32 sum)"""
    dy2 = dy.reshape(-1, dy.shape[-1])
    M, N = dy2.shape
    K = w.shape[1]
    if dx is None:
        dx = torch.empty(*dy.shape[:-1], K, device=dy.device, dtype=dy.dtype)
    d2 = dx.view(-1, K)
    p2 = pre.reshape(-1, K) if pre is not None else None
    r2 = residual.view(-1, K) if residual is not None else None
    gemm(dy2, w, d2, M=M, N=K, K=N, lda_m=dy2.stride(0), lda_k=1, ldb_k=K, ldb_n=1, ldc=K,
         aux=p2, ldx=K, aux_mode=2 if pre is not None else 0, act=ACT[act] if pre is not None else 0,
         alpha=alpha, beta=1.0 if accumulate else 0.0, residual=r2, ldr=K if r2 is not None else 0)
    return dx


def ffn_bwd_dgrad_ok(dy, w2, w1, hid):
    """s2h_ffn_bwd_dgrad applies: bf16, d_model 256, hidden a multiple of 128, rows a multiple of 64,
    contiguous weights, unit-stride 16-B aligned rows"""
    if dy.dim() != 2 or hid.dim() != 2:
        return False
    R, H = hid.shape
    return (all(t.dtype == torch.bfloat16 for t in (dy, w2, w1, hid)) and dy.shape == (R, 256)
            and tuple(w2.shape) == (256, H) and tuple(w1.shape) == (H, 256) and H % 128 == 0 and R % 64 == 0
            and w2.is_contiguous() and w1.is_contiguous() and hid.is_contiguous() and dy.stride(1) == 1
            and dy.stride(0) % 8 == 0 and R * max(H, dy.stride(0)) < 2**31
            and all(t.data_ptr() % 16 == 0 for t in (dy, w2, w1, hid)))


def ffn_bwd_dgrad(dy, w2, w1, hid, alpha=1.0, dh=None, dx=None):
    """Memory-attention FFN backward, input-gradient side, in one launch (csrc/ffn.hip):
    dh = alpha * (dy @ w2) * [hid > 0] (linear1's pre-activation gradient) and dx = dh @ w1.
    dy [R, 256], w2 [256, H] (linear2.weight), w1 [H, 256] (linear1.weight), hid [R, H] (linear2's
    saved input).  Returns (dh, dx)."""
    assert ffn_bwd_dgrad_ok(dy, w2, w1, hid)
    R, H = hid.shape
    if dh is None:
        dh = torch.empty(R, H, device=dy.device, dtype=dy.dtype)
    if dx is None:
        dx = torch.empty(R, 256, device=dy.device, dtype=dy.dtype)
    _dev(dy, w2, w1, hid, dh, dx)
    call("s2h_ffn_bwd_dgrad", R, H, ptr(dy), dy.stride(0), ptr(w2), ptr(w1), ptr(hid), H, float(alpha), ptr(dh),
         dh.stride(0), ptr(dx), dx.stride(0), stream())
    return dh, dx


def ffn_fwd_ok(x, w1, b1, w2, b2):
    """s2h_ffn_fwd applies: bf16, d_model 256, hidden 1024 or 2048, rows a multiple of 64,
    contiguous 16-B aligned operands, fp32 biases"""
    if x.dim() != 2:
        return False
    R, C = x.shape
    H = w1.shape[0]
    return (x.dtype == torch.bfloat16 and w1.dtype == torch.bfloat16 and w2.dtype == torch.bfloat16
            and b1 is not None and b2 is not None and b1.dtype == torch.float32 and b2.dtype == torch.float32
            and C == 256 and tuple(w1.shape) == (H, 256) and tuple(w2.shape) == (256, H) and H in (1024, 2048)
            and R % 64 == 0 and R * max(H, x.stride(0)) < 2**31 and x.stride(1) == 1 and x.stride(0) % 8 == 0
            and all(t.is_contiguous() for t in (w1, w2, b1, b2))
            and all(t.data_ptr() % 16 == 0 for t in (x, w1, w2, b1, b2)))


def ffn_fwd(x, w1, b1, w2, b2, p=0.0, seed1=0, idx1=0, seed2=0, idx2=0, hid=None, y=None):
    """Memory-attention FFN forward in one launch (csrc/ffn.hip): hid = drop(relu(x w1^T + b1)),
    y = drop(hid w2^T + b2) with the GEMM epilogue's dropout hash (seed1 / idx1, seed2 / idx2).
    Returns (hid, y)."""
    assert ffn_fwd_ok(x, w1, b1, w2, b2)
    R = x.shape[0]
    H = w1.shape[0]
    if hid is None:
        hid = torch.empty(R, H, device=x.device, dtype=x.dtype)
    if y is None:
        y = torch.empty(R, 256, device=x.device, dtype=x.dtype)
    assert hid.is_contiguous() and y.is_contiguous()
    _dev(x, w1, b1, w2, b2, hid, y)
    call("s2h_ffn_fwd", R, H, ptr(x), x.stride(0), ptr(w1), ptr(b1), ptr(w2), ptr(b2), float(p),
         int(seed1) & (2**64 - 1), int(idx1), int(seed2) & (2**64 - 1), int(idx2), ptr(hid), H, ptr(y), 256, stream())
    return hid, y


def linear_dgrad_ln_bwd_ok(dy, w, x):
    """s2h_linear_dgrad_ln_bwd applies: bf16, LayerNorm width 128 / 256, 16-B aligned rows"""
    K = w.shape[1]
    return (dy.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and x.dtype == torch.bfloat16 and K in (128, 256)
            and w.is_contiguous() and dy.shape[-1] % 8 == 0 and dy.stride(-1) == 1 and x.is_contiguous()
            and all(t.data_ptr() % 16 == 0 for t in (dy, w, x)))


def linear_dgrad_ln_bwd(dy, w, x, gamma, mean, rstd, dres=None, dgamma=None, dbeta=None, alpha=1.0, dx=None):
    """dx = LN'(alpha * dy @ w) + dres for a LayerNorm (input x, gamma, saved mean / rstd) whose output
    feeds only the Linear with weight w; dgamma / dbeta += its weight gradients -- one full-row GEMM
    launch with the LayerNorm backward in the epilogue (+ the partial-row finalize)"""
    dy2 = dy.reshape(-1, dy.shape[-1])
    M, N = dy2.shape
    C = w.shape[1]
    x2 = x.reshape(-1, C)
    assert x2.shape[0] == M and w.shape[0] == N and mean.numel() >= M and rstd.numel() >= M
    if dx is None:
        dx = torch.empty(x.shape, device=dy.device, dtype=dy.dtype)
    d2 = dx.view(-1, C)
    r2 = dres.reshape(-1, C) if dres is not None else None
    if r2 is not None:
        assert r2.stride(1) == 1 and r2.dtype == dx.dtype
    part = None
    if dgamma is not None:
        nbytes = lib().s2h_linear_dgrad_ln_bwd_ws_bytes(M, C)
        part = torch.empty(max(nbytes // 4, 1), device=dy.device, dtype=torch.float32)
    _dev(dy2, w, x2, gamma, mean, rstd, r2, d2, dgamma, dbeta)
    call("s2h_linear_dgrad_ln_bwd", M, C, N, ptr(dy2), dy2.stride(0), ptr(w), w.stride(0), float(alpha), ptr(x2), C,
         ptr(gamma), ptr(mean), ptr(rstd), ptr(r2), r2.stride(0) if r2 is not None else 0, ptr(d2), C, ptr(part),
         ptr(dgamma), ptr(dbeta), stream())
    return dx


def mlp_heads(heads, outs=None, hidden=None, pre=None):
    """MLP heads in one launch (s2h_mlp_heads): heads = [(x [M, K0] bf16 rows, [W_l] bf16 [N_l, K_l],
    [b_l fp32 or None], act_last)] with the same M; ReLU between layers.  outs: optional [y] to write;
    hidden: optional [[h_l]] per head (each hidden layer's ReLU output, contiguous); pre: optional
    [pre-activation of the last layer or None] per head.  Returns [y]"""
    import ctypes
    n = len(heads)
    M = heads[0][0].shape[0]
    xs, lds, ws, bs, dims, nls, acts, ys, ldys = [], [], [], [], [], [], [], [], []
    hids, pres = [], []
    for hi, (x, wl, bl, act_last) in enumerate(heads):
        assert x.dtype == torch.bfloat16 and x.shape[0] == M and x.stride(1) == 1 and len(wl) <= 3
        y = outs[hi] if outs is not None else torch.empty(M, wl[-1].shape[0], device=x.device, dtype=x.dtype)
        assert y.shape == (M, wl[-1].shape[0]) and y.stride(1) == 1
        hl = hidden[hi] if hidden is not None else []
        for h, w in zip(hl, wl[:-1]):
            assert h.is_contiguous() and h.shape == (M, w.shape[0])
        hids += [ptr(h) for h in hl] + [None] * (2 - len(hl))
        pl = pre[hi] if pre is not None else None
        assert pl is None or (pl.is_contiguous() and pl.shape == y.shape)
        pres.append(ptr(pl))
        _dev(x, y, *wl, *[b for b in bl if b is not None])
        xs.append(ptr(x))
        lds.append(x.stride(0))
        d = [x.shape[1]] + [w.shape[0] for w in wl]
        for w, k in zip(wl, d[:-1]):
            assert w.is_contiguous() and w.dtype == torch.bfloat16 and w.shape[1] == k
        dims += d + [0] * (4 - len(d))
        ws += [ptr(w) for w in wl] + [None] * (3 - len(wl))
        bs += [ptr(b) for b in bl] + [None] * (3 - len(bl))
        nls.append(len(wl))
        acts.append(ACT[act_last])
        ys.append(y)
        ldys.append(y.stride(0))
    P = ctypes.c_void_p
    call("s2h_mlp_heads", n, M, (P * n)(*xs), (ctypes.c_int64 * n)(*lds), (P * (3 * n))(*ws),
         (P * (3 * n))(*bs), (ctypes.c_int * (4 * n))(*dims), (ctypes.c_int * n)(*nls), (ctypes.c_int * n)(*acts),
         (P * n)(*[ptr(y) for y in ys]), (ctypes.c_int64 * n)(*ldys),
         (P * (2 * n))(*hids) if hidden is not None else None, (P * n)(*pres) if pre is not None else None, stream())
    return ys


def linear_wgrad(dy, x, dw, accumulate=True, db=None):
    """dw (fp32 [N, K]) (+)= dy^T @ x;  db (fp32 [N], optional) (+)= dy summed over rows."""
    dy2 = dy.reshape(-1, dy.shape[-1])
    x2 = x.reshape(-1, x.shape[-1])
    M, N = dy2.shape
    K = x2.shape[1]
    assert dw.dtype == torch.float32 and dw.shape == (N, K) and dw.stride(1) == 1
    assert dy2.dtype == x2.dtype and dy2.stride(1) == 1 and x2.stride(1) == 1
    if db is not None:
        assert db.dtype == torch.float32 and db.numel() == N and db.is_contiguous()
    _dev(dy2, x2, dw, db)
    if M >= 512 and "t" not in _WG_WS:
        wgrad_workspace(dw.device)
    call("s2h_linear_wgrad", dt(dy2), M, N, K, ptr(dy2), dy2.stride(0), ptr(x2), x2.stride(0), ptr(dw), dw.stride(0),
         ptr(db), int(accumulate), stream())
    return dw


# ----------------------------------------------------------------- MX-fp8 (config 5)
class MX8:
    """An MX-fp8 (OCP MXFP8-E4M3) operand as s2h_mx8_quant writes it: `q` [rows, Kp] uint8 e4m3
    codes (Kp = k rounded up to 128, zero padded), `s` [Kp / 128, rows] int32 scale words (byte b
    of word (kt, r) = E8M0 exponent of the 32-block 4kt + b of row r), `k` the logical depth."""
    __slots__ = ("q", "s", "k")

    def __init__(self, q, s, k):
        self.q, self.s, self.k = q, s, k

    @property
    def rows(self):
        return self.q.shape[0]


def mx8_empty(rows, k, device):
    kp = (k + 127) // 128 * 128
    return MX8(torch.empty(rows, kp, dtype=torch.uint8, device=device),
               torch.empty(kp // 128, rows, dtype=torch.int32, device=device), k)


def mx8_quant(x, out=None, transpose=False):
    """MX-fp8 of the rows of 2-D `x` [rows, cols] (blocks along cols, cols contiguous), or with
    transpose=True of x^T ([cols, rows] -> blocks along x's rows: the dgrad operand of a weight)."""
    _dev(x)
    assert x.dim() == 2
    if transpose:
        assert x.stride(0) == 1 or x.is_contiguous()
        rows, cols = x.shape[1], x.shape[0]
        ld_row, ld_col = x.stride(1), x.stride(0)
    else:
        assert x.stride(1) == 1
        rows, cols = x.shape
        ld_row, ld_col = x.stride(0), 1
    if out is None:
        out = mx8_empty(rows, cols, x.device)
    assert out.q.shape[0] == rows and out.k == cols and out.s.shape[1] >= rows
    call("s2h_mx8_quant", rows, cols, dt(x), ptr(x), ld_row, ld_col, ptr(out.q), out.q.stride(0), ptr(out.s),
         out.s.stride(0), stream())
    return out


def gemm_mx8(a: MX8, b: MX8, c, *, bias=None, residual=None, aux=None, aux_mode=0, act=0, drop_p=0.0, seed=0,
             drop_idx0=0, alpha=1.0, beta=0.0):
    """c[M, N] = epilogue(alpha * A B^T) for MX-fp8 A [M, K] and B [N, K] (s2h_gemm_mx8)"""
    assert a.k == b.k and c.dim() == 2 and c.stride(1) == 1
    M, N = a.rows, b.rows
    assert c.shape == (M, N)
    _operand_dtype("residual", residual, torch.bfloat16)
    _operand_dtype("aux", aux, torch.bfloat16)
    _dev(a.q, b.q, c, bias, residual, aux)
    call("s2h_gemm_mx8", M, N, a.k, ptr(a.q), a.q.stride(0), ptr(a.s), a.s.stride(0), ptr(b.q), b.q.stride(0),
         ptr(b.s), b.s.stride(0), ptr(c), dt(c), c.stride(0), ptr(bias), ptr(residual),
         residual.stride(0) if residual is not None else 0, ptr(aux), aux.stride(0) if aux is not None else 0,
         aux_mode if aux is not None else 0, float(drop_p), int(seed) & (2**64 - 1), int(drop_idx0), float(alpha),
         float(beta), int(act), stream())
    return c


def linear_mx8(x, w8: MX8, bias=None, act=None, out=None, pre=None, residual=None, drop_p=0.0, seed=0, drop_idx0=0):
    """ops.linear with MX-fp8 operands: x (bf16) quantised here, w8 = the weight's MX-fp8 copy."""
    x2 = x.reshape(-1, x.shape[-1])
    N = w8.rows
    assert x2.shape[1] == w8.k
    if out is None:
        out = torch.empty(*x.shape[:-1], N, device=x.device, dtype=x.dtype)
    xq = mx8_quant(x2 if x2.stride(1) == 1 else x2.contiguous())
    gemm_mx8(xq, w8, out.view(-1, N), bias=bias, residual=residual.reshape(-1, N) if residual is not None else None,
             aux=pre.view(-1, N) if pre is not None else None, aux_mode=1 if pre is not None else 0, act=ACT[act],
             drop_p=drop_p, seed=seed, drop_idx0=drop_idx0)
    return out


def linear_dgrad_mx8(dy, wt8: MX8, dx=None, accumulate=False, pre=None, act=None, alpha=1.0):
    """ops.linear_dgrad with MX-fp8 operands: dy quantised along its N, wt8 = MX-fp8 of W^T [K, N]."""
    dy2 = dy.reshape(-1, dy.shape[-1])
    K = wt8.rows
    assert dy2.shape[1] == wt8.k
    if dx is None:
        dx = torch.empty(*dy.shape[:-1], K, device=dy.device, dtype=dy.dtype)
    dq = mx8_quant(dy2 if dy2.stride(1) == 1 else dy2.contiguous())
    gemm_mx8(dq, wt8, dx.view(-1, K), aux=pre.reshape(-1, K) if pre is not None else None,
             aux_mode=2 if pre is not None else 0, act=ACT[act] if pre is not None else 0, alpha=alpha,
             beta=1.0 if accumulate else 0.0)
    return dx


def bmm(a, b, out, *, trans_b=False, alpha=1.0, beta=0.0):
    """Batched out[i] = a[i] @ b[i] (or b[i]^T): a [Bt, M, K], b [Bt, K, N] / [Bt, N, K]."""
    Bt, M, K = a.shape
    if trans_b:
        N = b.shape[1]
        ldb_k, ldb_n = b.stride(2), b.stride(1)
    else:
        N = b.shape[2]
        ldb_k, ldb_n = b.stride(1), b.stride(2)
    gemm(a, b, out, M=M, N=N, K=K, lda_m=a.stride(1), lda_k=a.stride(2), ldb_k=ldb_k, ldb_n=ldb_n,
         ldc=out.stride(1), batch=Bt, sA=a.stride(0), sB=b.stride(0), sC=out.stride(0), alpha=alpha, beta=beta)
    return out


# ------------------------------------------------------------ attention
def _bhl(t):
    """strides (batch, head, row) of a [B, L, H, D] view with contiguous D"""
    assert t.stride(3) == 1
    return t.stride(0), t.stride(2), t.stride(1)


def keep_bits_ok(q, p_drop):
    """the flash forward writes (and the flash backward reads) a dropout keep bitmap for this
    attention: dropout on, bf16 head_dim 256 flash path"""
    return p_drop > 0 and q.shape[-1] == 256 and flash_bwd_eligible(q)


def keep_words(B, H, Lq, Lk):
    """int32 words of one launch's keep bitmap (s2h_attn_keep_words)"""
    return B * H * Lq * 2 * ((Lk + 63) // 64)


def attn_fwd(q, k, v, o, lse, scale, p_drop=0.0, seed=0, idx0=0, keep=None):
    """q [B, Lq, H, D], k/v [B, Lk, H, D] (any strides, D contiguous) -> o [B, Lq, H, D], lse [B, H, Lq] f32;
    keep: optional int32 [keep_words(...)] receiving the dropout keep bitmap (keep_bits_ok)"""
    _dev(q, k, v, o, lse)
    B, Lq, H, D = q.shape
    Lk = k.shape[1]
    nws = lib().s2h_attn_fwd_ws_bytes(dt(q), B, H, Lq, Lk, D)
    ws = torch.empty(nws, device=q.device, dtype=torch.uint8) if nws > 0 else None
    call("s2h_attn_fwd", dt(q), B, H, Lq, Lk, D, ptr(q), *_bhl(q), ptr(k), *_bhl(k), ptr(v), *_bhl(v),
         ptr(o), *_bhl(o), ptr(lse), float(scale), float(p_drop), int(seed) & (2**64 - 1), int(idx0),
         _keep_ptr(keep, B, H, Lq, Lk), ptr(ws), int(nws), stream())
    return o, lse


VFOLD_DV, VFOLD_COLS = 64, 72  # memory channels; columns of u' = [D M | rowsum(D) | 0 x 7]


def vfold_ok(q, mem):
    """the folded cross-attention's domain: bf16, one head of dim 256 (q [B, Lq, 1, 256]), 64-channel
    memory, flash-eligible query count"""
    return (q.dtype == torch.bfloat16 and q.shape[-1] == 256 and q.shape[-2] == 1 and mem.shape[-1] == VFOLD_DV
            and bool(lib().s2h_flash_bwd_ok(BF16, q.shape[1], 256)))


def _brs(t):
    """(batch, row) strides of a [B, L, (1,) C] view with contiguous channels"""
    assert t.stride(-1) == 1
    return t.stride(0), t.stride(1)


def attn_fwd_vfold(q, k, mem, u, lse, scale, p_drop=0.0, seed=0, idx0=0, keep=None):
    """q [B, Lq, 1, 256], k [B, Lk, 1, 256], mem [B, Lk, 1, 64] -> u [B, Lq, 1, 72] (u' = [D mem |
    rowsum(D) | 0]), lse [B, 1, Lq] (s2h_attn_fwd_vfold); keep as attn_fwd"""
    _dev(q, k, mem, u, lse)
    B, Lq = q.shape[0], q.shape[1]
    Lk = k.shape[1]
    nws = lib().s2h_attn_fwd_vfold_ws_bytes(B, Lq, Lk)
    ws = torch.empty(nws, device=q.device, dtype=torch.uint8) if nws > 0 else None
    call("s2h_attn_fwd_vfold", B, Lq, Lk, ptr(q), *_brs(q), ptr(k), *_brs(k), ptr(mem), *_brs(mem), ptr(u),
         *_brs(u), ptr(lse), float(scale), float(p_drop), int(seed) & (2**64 - 1), int(idx0),
         _keep_ptr(keep, B, 1, Lq, Lk), ptr(ws), int(nws), stream())
    return u, lse


def _rope_table_args(nfr, rope):
    """(cos, sin, period) checks and the per-frame row-count arrays of a fused inverse RoPE"""
    import ctypes
    cos, sin, period = rope[:3]
    _dev(cos, sin)
    assert cos.dtype == sin.dtype == torch.float32 and cos.is_contiguous() and sin.is_contiguous()

    def arr(n):  # (address, the ctypes array that must outlive the call)
        if n is None:
            return None
        assert len(n) == nfr
        a = (ctypes.c_int * nfr)(*[int(x) for x in n])
        return ctypes.addressof(a), a
    return ptr(cos), ptr(sin), int(period), arr


def flash_bwd_frames_vfold(nfr, bpf, lk, krow, idx0, q, k, mem, u, du, lse, dq, dk, scale, p_drop, seed, keep=None,
                           koff=None, rope=None, rope_q=None):
    """Frame-batched backward of attn_fwd_vfold (s2h_flash_bwd_frames_vfold): q / u / du / dq
    [nfr*bpf, Lq, 1, C] views, k / mem / dk PACKED [rows, 1, C] (frame f: bpf blocks of lk[f] rows
    from row krow[f]); keep / koff as flash_bwd_frames.  rope = (cos, sin, period, nrot per frame or
    None): dk comes out rotated back (the k projection's RoPE transposed, fused into the dK store);
    rope_q = query rows rotated per frame (same tables): dq rotated back in the dQ store
    (s2h_flash_bwd_frames_vfold_rope_qk)"""
    import ctypes
    _dev(q, k, mem, u, du, lse, dq, dk)
    B, Lq = q.shape[0], q.shape[1]
    assert B == nfr * bpf and len(lk) == nfr == len(krow) == len(idx0)
    di = torch.empty(B * Lq, device=q.device, dtype=torch.float32)
    alk = (ctypes.c_int * nfr)(*[int(x) for x in lk])
    akr = (ctypes.c_int64 * nfr)(*[int(x) for x in krow])
    aix = (ctypes.c_uint64 * nfr)(*[int(x) & (2**64 - 1) for x in idx0])
    kp = ako = None
    if keep is not None:
        assert keep.dtype == torch.int32 and len(koff) == nfr
        assert all(int(koff[f]) + keep_words(bpf, 1, Lq, lk[f]) <= keep.numel() for f in range(nfr))
        ako = (ctypes.c_int64 * nfr)(*[int(x) for x in koff])
        kp = ptr(keep)

    def rs(t):  # row stride of a packed [rows, 1, C] view
        assert t.stride(-1) == 1
        return t.stride(0)
    args = [nfr, bpf, Lq, ctypes.cast(alk, ctypes.c_void_p).value, ctypes.cast(akr, ctypes.c_void_p).value,
            ctypes.cast(aix, ctypes.c_void_p).value, ptr(q), *_brs(q), ptr(k), rs(k), ptr(mem), rs(mem), ptr(u), *_brs(u),
            ptr(du), *_brs(du), ptr(dq), *_brs(dq), ptr(dk), rs(dk), ptr(lse), ptr(di), float(scale), float(p_drop),
            int(seed) & (2**64 - 1), kp, ctypes.cast(ako, ctypes.c_void_p).value if kp is not None else None]
    if rope is None:
        assert rope_q is None
        call("s2h_flash_bwd_frames_vfold", *args, stream())
    else:
        pc, ps, period, arr = _rope_table_args(nfr, rope)
        ank, anq = arr(rope[3]), arr(rope_q)  # (pointer, keep-alive list)
        call("s2h_flash_bwd_frames_vfold_rope_qk", *args, pc, ps, period, ank[0] if ank else None,
             anq[0] if anq else None, stream())
    return dq, dk


def vfold_weight(wv, bv, out=None):
    """[Wv | bv | 0] bf16 [N, 72] from the bf16 weight [N, 64] and the fp32 bias [N]"""
    N, K = wv.shape
    if out is None:
        out = torch.empty(N, VFOLD_COLS, device=wv.device, dtype=torch.bfloat16)
    assert wv.dtype == torch.bfloat16 and wv.is_contiguous() and bv.dtype == torch.float32 and out.is_contiguous()
    call("s2h_vfold_weight", N, K, out.shape[1], ptr(wv), ptr(bv), ptr(out), stream())
    return out


def vfold_grad(g, gwv, gbv):
    """gwv [N, K] += g[:, :K], gbv [N] += g[:, K] (g fp32 [N, ld])"""
    N, ld = g.shape
    K = gwv.shape[1] if gwv is not None else VFOLD_DV
    call("s2h_vfold_grad", N, K, ld, ptr(g), ptr(gwv), ptr(gbv), stream())


def _keep_ptr(keep, B, H, Lq, Lk):
    if keep is None:
        return None
    assert keep.dtype == torch.int32 and keep.is_contiguous() and keep.numel() >= keep_words(B, H, Lq, Lk)
    return ptr(keep)


def attn_bwd(q, k, v, o, do, lse, dq, dk, dv, scale, p_drop=0.0, seed=0, idx0=0, keep=None):
    _dev(q, k, v, o, do, lse, dq, dk, dv)
    B, Lq, H, D = q.shape
    Lk = k.shape[1]
    di = torch.empty(B * H * Lq, device=q.device, dtype=torch.float32)
    nws = lib().s2h_attn_bwd_ws_bytes(dt(q), B, H, Lq, Lk, D)
    ws = torch.empty(nws, device=q.device, dtype=torch.uint8) if nws > 0 else None
    call("s2h_attn_bwd", dt(q), B, H, Lq, Lk, D,
         ptr(q), *_bhl(q), ptr(k), *_bhl(k), ptr(v), *_bhl(v), ptr(o), *_bhl(o), ptr(do), *_bhl(do),
         ptr(dq), *_bhl(dq), ptr(dk), *_bhl(dk), ptr(dv), *_bhl(dv),
         ptr(lse), ptr(di), float(scale), float(p_drop), int(seed) & (2**64 - 1), int(idx0),
         _keep_ptr(keep, B, H, Lq, Lk), ptr(ws), int(nws), stream())
    return dq, dk, dv


def flash_bwd_eligible(q):
    """the frame-batched flash backward's domain (bf16, head_dim 32..128 / 256, >= 128 query rows,
    flash path enabled): q [B, Lq, H, D]"""
    return bool(lib().s2h_flash_bwd_ok(dt(q), q.shape[1], q.shape[-1]))


def flash_bwd_frames(nfr, bpf, lk, krow, idx0, q, k, v, o, do, lse, dq, dk, dv, scale, p_drop, seed, keep=None,
                     koff=None, rope=None):
    """Frame-batched flash backward (s2h_flash_bwd_frames): q/o/do/dq [nfr*bpf, Lq, H, D] views,
    k/v/dk/dv PACKED [rows, H, D] views (frame f: bpf blocks of lk[f] rows from row krow[f]),
    lse [nfr*bpf, H, Lq]; frame f's dropout indices start at idx0[f]; keep (optional int32) holds
    frame f's forward keep bitmap from word koff[f].  rope = (cos, sin, period, query rows per frame):
    dq comes out rotated back (s2h_flash_bwd_frames_rope, the q projection's RoPE transposed in the
    dQ store; head dim 256)"""
    import ctypes
    _dev(q, k, v, o, do, lse, dq, dk, dv)
    B, Lq, H, D = q.shape
    assert B == nfr * bpf and len(lk) == nfr == len(krow) == len(idx0)
    di = torch.empty(B * H * Lq, device=q.device, dtype=torch.float32)
    alk = (ctypes.c_int * nfr)(*[int(x) for x in lk])
    akr = (ctypes.c_int64 * nfr)(*[int(x) for x in krow])
    aix = (ctypes.c_uint64 * nfr)(*[int(x) & (2**64 - 1) for x in idx0])
    kp = None
    if keep is not None:
        assert keep.dtype == torch.int32 and len(koff) == nfr
        assert all(int(koff[f]) + keep_words(bpf, H, Lq, lk[f]) <= keep.numel() for f in range(nfr))
        ako = (ctypes.c_int64 * nfr)(*[int(x) for x in koff])
        kp = ptr(keep)

    def hl(t):  # (head, row) strides of a packed [rows, H, D] view
        assert t.stride(-1) == 1
        return t.stride(1), t.stride(0)
    args = [nfr, bpf, H, Lq, D, ctypes.cast(alk, ctypes.c_void_p).value, ctypes.cast(akr, ctypes.c_void_p).value,
            ctypes.cast(aix, ctypes.c_void_p).value, ptr(q), *_bhl(q), ptr(k), *hl(k), ptr(v), *hl(v), ptr(o),
            *_bhl(o), ptr(do), *_bhl(do), ptr(dq), *_bhl(dq), ptr(dk), *hl(dk), ptr(dv), *hl(dv), ptr(lse), ptr(di),
            float(scale), float(p_drop), int(seed) & (2**64 - 1), kp,
            ctypes.cast(ako, ctypes.c_void_p).value if kp is not None else None]
    if rope is None:
        call("s2h_flash_bwd_frames", *args, stream())
    else:
        pc, ps, period, arr = _rope_table_args(nfr, rope)
        anq = arr(rope[3])
        call("s2h_flash_bwd_frames_rope", *args, pc, ps, period, anq[0], stream())
    return dq, dk, dv


# ------------------------------------------------------------ layernorm
def layernorm_fwd(x, gamma, beta, eps, y=None, add=None, add_bcast=False, xsum=None):
    """y = LN(x [+ add]) over the last dim; returns (y, mean, rstd).  If add is given the
    sum is written to xsum (residual stream)."""
    rows, C = _rows(x)
    if y is None:
        y = torch.empty(x.shape, device=x.device, dtype=x.dtype)
    mean = torch.empty(rows, device=x.device, dtype=torch.float32)
    rstd = torch.empty(rows, device=x.device, dtype=torch.float32)
    call("s2h_layernorm_fwd", dt(x), rows, C, ptr(x), x.stride(-2) if x.dim() > 1 else C,
         ptr(add), (add.stride(-2) if (add is not None and add.dim() > 1) else C), int(add_bcast), ptr(xsum),
         ptr(gamma), ptr(beta), float(eps), ptr(y), C, ptr(mean), ptr(rstd), stream())
    return y, mean, rstd


def layernorm_bwd(x, dy, gamma, mean, rstd, dx=None, accumulate=False, dgamma=None, dbeta=None, dres=None):
    """dx = LN'(dy) (+ dx when accumulate, or + dres); dgamma/dbeta += weight gradients."""
    rows, C = _rows(x)
    if dx is None:
        dx = torch.empty(x.shape, device=x.device, dtype=x.dtype)
    if dres is not None:
        assert dres.is_contiguous() and dres.dtype == x.dtype and dres.numel() == x.numel() and not accumulate
    ws = None
    if dgamma is not None:  # (unused when the library defers the gamma / beta sums)
        nbytes = lib().s2h_layernorm_bwd_ws_bytes(dt(x), rows, C)
        ws = torch.empty(max(nbytes // 4, 1), device=x.device, dtype=torch.float32)
    call("s2h_layernorm_bwd", dt(x), rows, C, ptr(x), C, ptr(dy), C, ptr(gamma), ptr(mean), ptr(rstd),
         ptr(dx), C, int(accumulate), ptr(dres), C, ptr(dgamma), ptr(dbeta), ptr(ws), stream())
    return dx


# ----------------------------------------------------------- elementwise
def add(a, b, out=None, alpha=1.0, beta=1.0):
    ref = a if a is not None else b
    if out is None:
        out = torch.empty_like(ref)
    call("s2h_add", dt(ref), ref.numel(), ptr(a), ptr(b), float(alpha), float(beta), ptr(out), stream())
    return out


def add_bcast(a, b, out=None, alpha=1.0, beta=1.0, b_period=1, shape=None):
    """out[i, :] = alpha*a[i, :] + beta*b[i % b_period, :]  (a may be None -> broadcast copy)"""
    inner = b.numel() // b_period
    if out is None:
        out = torch.empty(shape if shape is not None else a.shape, device=b.device, dtype=b.dtype)
    outer = out.numel() // inner
    call("s2h_add_bcast", dt(out), outer, inner, ptr(a), float(alpha), ptr(b), b_period, float(beta), ptr(out),
         stream())
    return out


def act_fwd(x, act, out=None, scale=1.0, shift=0.0):
    if out is None:
        out = torch.empty_like(x)
    call("s2h_act_fwd", dt(x), x.numel(), ptr(x), ACT[act], float(scale), float(shift), ptr(out), stream())
    return out


def act_dropout_bwd(x_pre, dy, act, p, seed, dx=None, idx0=0):
    """dx = act'(x_pre) * dropout_mask(seed) / (1 - p) * dy (one pass; x_pre None = no act)"""
    if dx is None:
        dx = torch.empty_like(dy)
    call("s2h_act_dropout_bwd", dt(dy), dy.numel(), ptr(x_pre), ptr(dy), ACT[act], float(p), int(seed) & (2**64 - 1),
         int(idx0), ptr(dx), stream())
    return dx


def relu_mask_bwd(y, dy, scale=1.0, dx=None):
    """dx = scale * [y > 0] * dy -- ReLU (-> dropout) backward from the layer output y"""
    assert y.is_contiguous() and dy.is_contiguous() and y.numel() == dy.numel() and y.dtype == dy.dtype
    if dx is None:
        dx = torch.empty_like(dy)
    call("s2h_relu_mask_bwd", dt(dy), dy.numel(), ptr(y), ptr(dy), float(scale), ptr(dx), stream())
    return dx


def act_bwd(x_pre, dy, act, dx=None, accumulate=False):
    if dx is None:
        dx = torch.empty_like(dy)
    call("s2h_act_bwd", dt(dy), dy.numel(), ptr(x_pre), ptr(dy), ACT[act], ptr(dx), int(accumulate), stream())
    return dx


def cast(x, dtype, out=None):
    if out is None:
        out = torch.empty(x.shape, device=x.device, dtype=dtype)
    call("s2h_cast", dt(x), dt(out), x.numel(), ptr(x), ptr(out), stream())
    return out


def dropout(b, p, seed, a=None, out=None, idx0=0):
    """out = (a +) keep*b/(1-p) with the counter-hash mask of (seed, flat index)"""
    if out is None:
        out = torch.empty_like(b)
    call("s2h_dropout", dt(b), b.numel(), ptr(a), ptr(b), float(p), int(seed) & (2**64 - 1), int(idx0), ptr(out),
         stream())
    return out


def rope(x, y, nrot, cos, sin, period, inverse=False):
    """x/y [Bt, L, D] views (D contiguous): rotate pairs of the first nrot rows of every batch."""
    Bt, L, D = x.shape
    call("s2h_rope", dt(x), Bt, nrot, D, ptr(x), x.stride(0), x.stride(1), ptr(y), y.stride(0), y.stride(1),
         ptr(cos), ptr(sin), period, int(inverse), stream())
    return y


def maxpool2(x, out=None):
    """x [B, H, W, C] (pixel stride x.stride(2), C contiguous) -> [B, H/2, W/2, C]"""
    B, H, W, C = x.shape
    assert x.stride(1) == W * x.stride(2) and x.stride(0) == H * x.stride(1) and x.stride(3) == 1
    if out is None:
        out = torch.empty(B, H // 2, W // 2, C, device=x.device, dtype=x.dtype)
    call("s2h_maxpool2_fwd", dt(x), B, H, W, C, ptr(x), x.stride(2), ptr(out), stream())
    return out


def maxpool2_bwd(x, dy, dx):
    B, H, W, C = x.shape
    call("s2h_maxpool2_bwd", dt(x), B, H, W, C, ptr(x), x.stride(2), ptr(dy), ptr(dx), dx.stride(2), stream())
    return dx


def window_partition(x, ws, out=None, accumulate=False):
    B, H, W, C = x.shape
    nh, nw = -(-H // ws), -(-W // ws)
    if out is None:
        out = torch.empty(B * nh * nw, ws, ws, C, device=x.device, dtype=x.dtype)
    call("s2h_window", dt(x), B, H, W, C, ws, ptr(x), ptr(out), 0, int(accumulate), stream())
    return out


def window_pad(x, ws, padrow, out=None):
    """window_partition of a projection's output x [B, H, W, C] with the padded positions = padrow
    (fp32 [C], the projection's bias): [B * nh * nw, ws, ws, C]"""
    B, H, W, C = x.shape
    nh, nw = -(-H // ws), -(-W // ws)
    assert padrow.dtype == torch.float32 and padrow.numel() == C and padrow.is_contiguous() and x.is_contiguous()
    if out is None:
        out = torch.empty(B * nh * nw, ws, ws, C, device=x.device, dtype=x.dtype)
    _dev(x, padrow, out)
    call("s2h_window_pad", dt(x), B, H, W, C, ws, ptr(x), ptr(padrow), ptr(out), stream())
    return out


def window_pad_colsum(win, ws, B, H, W, out):
    """out (fp32 [C]) += the column sums of win's padded rows (window_pad's bias gradient)"""
    C = win.shape[-1]
    assert out.dtype == torch.float32 and out.numel() == C and out.is_contiguous() and win.is_contiguous()
    _dev(win, out)
    call("s2h_window_pad_colsum", dt(win), B, H, W, C, ws, ptr(win), ptr(out), stream())
    return out


# Padded-window attention straight from the image layout (csrc/flash.hip s2h_flash_win_fwd): the row
# map of a geometry is built (and range-checked) by the library on the host, uploaded once per device
# and kept for the life of the process, like the zero row the backward reads as a padded query's dO.
_WIN_MAPS = {}
_WIN_ZERO = {}


def window_map_host(H, W, ws):
    """the host row map of geometry (H, W, ws) as numpy int32 arrays (row [nW, L], padidx [nW, L],
    sets [nW]): row = token index y * W + x of window position l = iy * ws + ix or -1 for padding,
    padidx = the padded position's row in window_pad_colsum's order or -1, sets = bit s set when
    positions 16 s .. 16 s + 15 hold a token (s2h_window_map; raises if an entry is out of range)"""
    n = int(lib().s2h_window_map_len(int(H), int(W), int(ws)))
    if n <= 0:
        raise ValueError(f"window map of ({H}, {W}, {ws})")
    buf = np.empty(n, dtype=np.int32)
    call("s2h_window_map", int(H), int(W), int(ws), buf.ctypes.data, n)
    nW, L = (-(-H // ws)) * (-(-W // ws)), ws * ws
    return buf[:nW * L].reshape(nW, L), buf[nW * L:2 * nW * L].reshape(nW, L), buf[2 * nW * L:]


def window_map(H, W, ws, device):
    """the device copy of s2h_window_map(H, W, ws) (int32, [row | padidx | sets]); first use of a
    geometry must come before a graph capture (the warm-up steps do)"""
    d = _device_of(device)
    key = (int(H), int(W), int(ws), d)
    t = _WIN_MAPS.get(key)
    if t is None:
        row, pad, sets = window_map_host(H, W, ws)
        t = _persistent_alloc("window_map", row.size + pad.size + sets.size, torch.int32, d)
        t.copy_(torch.from_numpy(np.concatenate([row.ravel(), pad.ravel(), sets])))
        _WIN_MAPS[key] = t
    return t


def _win_zero_row(n, device):
    d = _device_of(device)
    t = _WIN_ZERO.get(d)
    if t is None or t.numel() < n:
        t = _persistent_alloc("window_zero_row", max(n, 128), torch.bfloat16, d)
        t.zero_()
        _WIN_ZERO[d] = t
    return t


def flash_win_ok(qkv, ws, nh):
    """the padded-window mode takes qkv [B, H, W, 3 d] (d = nh heads x hd): bf16, contiguous, the
    flash domain, 16-B aligned rows, per-image extents within the kernels' 32-bit offsets, enough
    batch-heads that the partitioned launches would run without a key split"""
    if not (qkv.is_cuda and qkv.dtype == torch.bfloat16 and qkv.dim() == 4 and qkv.is_contiguous()):
        return False
    B, H, W, d3 = qkv.shape
    if d3 % (3 * nh) or qkv.data_ptr() % 16:
        return False
    return bool(lib().s2h_flash_win_ok(BF16, B, H, W, int(ws), int(nh), d3 // 3 // nh))


def flash_win_fwd(qkv, ws, nh, padrow, scale):
    """qkv [B, H, W, 3 d] bf16, padrow [3 d] bf16 (the projection's bias) -> o [B, H, W, d], lse
    [B * nW * nh, L] (+inf at padded positions)"""
    B, H, W, d3 = qkv.shape
    d = d3 // 3
    nW, L = (-(-H // ws)) * (-(-W // ws)), ws * ws
    assert padrow.dtype == torch.bfloat16 and padrow.numel() == d3 and padrow.is_contiguous()
    m = window_map(H, W, ws, qkv.device)
    _win_zero_row(d // nh, qkv.device)  # the backward's, allocated outside any capture
    o = torch.empty(B, H, W, d, device=qkv.device, dtype=qkv.dtype)
    lse = torch.empty(B * nW * nh, L, device=qkv.device, dtype=torch.float32)
    _dev(qkv, padrow, o, lse)
    call("s2h_flash_win_fwd", B, H, W, int(ws), int(nh), d // nh, ptr(qkv), ptr(padrow), ptr(m), ptr(o), ptr(lse),
         float(scale), stream())
    return o, lse


def flash_win_bwd(qkv, ws, nh, padrow, o, do, lse, scale):
    """-> dqkv [B, H, W, 3 d] (dq | dk | dv of the real tokens), dpad [B * P, 2 d] (dk | dv of the
    padded keys, P per image, window_pad_colsum's order)"""
    B, H, W, d3 = qkv.shape
    d = d3 // 3
    nhw, nww = -(-H // ws), -(-W // ws)
    nW, L, P = nhw * nww, ws * ws, nhw * ws * nww * ws - H * W
    assert do.is_contiguous() and do.shape == o.shape and do.dtype == o.dtype
    m = window_map(H, W, ws, qkv.device)
    z = _win_zero_row(d // nh, qkv.device)
    dqkv = torch.empty_like(qkv)
    dpad = torch.empty(B * P, 2 * d, device=qkv.device, dtype=qkv.dtype)
    di = torch.empty(B * nW * nh * L, device=qkv.device, dtype=torch.float32)
    _dev(qkv, padrow, o, do, lse, dqkv, dpad)
    call("s2h_flash_win_bwd", B, H, W, int(ws), int(nh), d // nh, ptr(qkv), ptr(padrow), ptr(z), ptr(m), ptr(o), ptr(do),
         ptr(dqkv), ptr(dpad), ptr(lse), ptr(di), float(scale), stream())
    return dqkv, dpad


def pad_rows_colsum(dpad, B, P, out):
    """out (fp32 [C]) += the column sums of dpad [B * P, C] (bf16): window_pad_colsum over compact rows"""
    C = dpad.shape[-1]
    assert out.dtype == torch.float32 and out.numel() == C and out.is_contiguous() and dpad.is_contiguous()
    assert dpad.dtype == torch.bfloat16 and dpad.shape[0] == B * P
    _dev(dpad, out)
    call("s2h_pad_rows_colsum", B, P, C, ptr(dpad), ptr(out), stream())
    return out


def window_unpartition(win, ws, B, H, W, out=None, accumulate=False):
    C = win.shape[-1]
    if out is None:
        out = torch.empty(B, H, W, C, device=win.device, dtype=win.dtype)
    call("s2h_window", dt(win), B, H, W, C, ws, ptr(win), ptr(out), 1, int(accumulate), stream())
    return out


# S2H_COPY_BATCH=0: one Tensor.copy_ per pair (A/B of s2h_copy2d_batch)
_COPY_BATCH = os.environ.get("S2H_COPY_BATCH", "1") != "0"


def _pair_rows(src, dst):
    """(rows, row_bytes, src_pitch, dst_pitch) of the copy dst <- src (same shape and dtype) as a
    2-D byte copy, or None when the layouts do not reduce to one (contiguous rows, uniform pitch)"""
    if src.shape != dst.shape or src.dtype != dst.dtype:
        return None
    dims = [d for d in range(src.dim()) if src.shape[d] != 1]
    es = src.element_size()
    inner, k = 1, len(dims)
    while k > 0 and src.stride(dims[k - 1]) == inner and dst.stride(dims[k - 1]) == inner:
        inner *= src.shape[dims[k - 1]]
        k -= 1
    lead = dims[:k]
    if not lead:
        return 1, inner * es, inner * es, inner * es
    rows = 1
    for a, b in zip(lead[:-1], lead[1:]):  # the leading dims must collapse into one pitch
        if src.stride(a) != src.stride(b) * src.shape[b] or dst.stride(a) != dst.stride(b) * dst.shape[b]:
            return None
    for d in lead:
        rows *= src.shape[d]
    return rows, inner * es, src.stride(lead[-1]) * es, dst.stride(lead[-1]) * es


def copy_segments(pairs):
    """dst.copy_(src) for every (src, dst) pair, up to 16 pairs per launch (s2h_copy2d_batch): the
    memory bank assembly of a tracked frame (sam2_base.py:649-676) and the tracking loop's gradient
    packing.  A pair whose layout is not a 4-B aligned 2-D copy goes through Tensor.copy_ (16-B
    aligned pairs move in 16-B pieces, the rest in 4-B pieces)."""
    import ctypes
    if not _COPY_BATCH:
        for src, dst in pairs:
            dst.copy_(src)
        return
    segs = []
    for src, dst in pairs:
        r = _pair_rows(src, dst) if src.is_cuda and dst.is_cuda else None
        if r is None or src.numel() == 0 or any(v % 4 for v in r[1:]) or src.data_ptr() % 4 or dst.data_ptr() % 4 \
                or (r[0] > 1 and r[3] < r[1]):  # overlapping destination rows (a source pitch of 0 broadcasts)
            dst.copy_(src)
            continue
        segs.append((src.data_ptr(), dst.data_ptr()) + r)
    for i in range(0, len(segs), 16):
        chunk = segs[i:i + 16]
        n = len(chunk)
        P, L = ctypes.c_void_p * n, ctypes.c_int64 * n
        arrs = [P(*[c[0] for c in chunk]), P(*[c[1] for c in chunk])] + [L(*[c[j] for c in chunk]) for j in range(2, 6)]
        call("s2h_copy2d_batch", n, *arrs, stream())


def up2_add(lat, prev, out=None):
    B, H, W, C = lat.shape
    if out is None:
        out = torch.empty_like(lat)
    call("s2h_up2_add", dt(lat), B, H, W, C, ptr(lat), ptr(prev), ptr(out), stream())
    return out


def pool2_sum(dout, dprev, accumulate=False):
    B, Ho, Wo, C = dprev.shape
    call("s2h_pool2_sum", dt(dout), B, Ho, Wo, C, ptr(dout), ptr(dprev), int(accumulate), stream())
    return dprev


def bilinear(x, ho, wo, out=None):
    """x [N, hi, wi] f32 -> [N, ho, wo] (align_corners=False)"""
    N, hi, wi = x.shape
    if out is None:
        out = torch.empty(N, ho, wo, device=x.device, dtype=torch.float32)
    call("s2h_bilinear_fwd", N, hi, wi, ho, wo, ptr(x), ptr(out), stream())
    return out


def bilinear_bwd(dy, hi, wi, dx=None):
    N, ho, wo = dy.shape
    if dx is None:
        dx = torch.empty(N, hi, wi, device=dy.device, dtype=torch.float32)
    call("s2h_bilinear_bwd", N, hi, wi, ho, wo, ptr(dy), ptr(dx), stream())
    return dx


def colsum(x, out, accumulate=True):
    """out (fp32 [C]) (+)= x.reshape(-1, C).sum(0)"""
    rows, C = _rows(x)
    call("s2h_colsum", dt(x), rows, C, ptr(x), x.stride(-2) if x.dim() > 1 else C, ptr(out), int(accumulate),
         stream())
    return out


def colsum_seg(x, rows, offs, dsts, out):
    """out[dsts[s]] += x[offs[s]:offs[s] + rows].sum(0) for every segment s (x [R, C] row-contiguous,
    out fp32 [*, C]); one launch for up to 64 segments"""
    import ctypes
    C = x.shape[-1]
    _dev(x, out)
    assert x.stride(-1) == 1 and out.dtype == torch.float32 and out.is_contiguous() and len(offs) == len(dsts) <= 64
    o = (ctypes.c_int64 * len(offs))(*[int(v) for v in offs])
    d = (ctypes.c_int * len(dsts))(*[int(v) for v in dsts])
    call("s2h_colsum_seg", dt(x), len(offs), int(rows), C, ptr(x), x.stride(-2), ctypes.addressof(o),
         ctypes.addressof(d), ptr(out), stream())
    return out


def memory_pos(pos, tpos, idx, out):
    """out[j * L + l] = pos[l] + tpos[idx[j]] for j < len(idx) <= 16 (pos [L, C], tpos [*, C], out [n L, C],
    all contiguous, one dtype)"""
    import ctypes
    L, C = pos.shape
    _dev(pos, tpos, out)
    assert pos.is_contiguous() and tpos.is_contiguous() and out.is_contiguous() and len(idx) <= 16
    assert pos.dtype == tpos.dtype == out.dtype and out.numel() == len(idx) * L * C
    ix = (ctypes.c_int * len(idx))(*[int(v) for v in idx])
    call("s2h_memory_pos", dt(out), len(idx), L, C, ptr(pos), ptr(tpos), ctypes.addressof(ix), ptr(out), stream())
    return out


def sum_outer(x, out, accumulate=False):
    """out[j] = sum_o x[o, j]  (same dtype as x)"""
    O = x.shape[0]
    call("s2h_sum_outer", dt(x), O, x.numel() // O, ptr(x), ptr(out), int(accumulate), stream())
    return out


def sum_outer_batched(x3, out, accumulate=False):
    """out[f] (+)= x3[f].sum(0) for x3 [F, O, inner] (one launch; the values of F sum_outer calls)"""
    F, O, inner = x3.shape
    assert x3.is_contiguous() and out.is_contiguous() and out.numel() == F * inner and out.dtype == x3.dtype
    call("s2h_sum_outer_batched", dt(x3), F, O, inner, ptr(x3), ptr(out), int(accumulate), stream())
    return out


def im2col(x, kh, kw, stride, pad, pad8=False):
    """[B*Ho*Wo, C*kh*kw] patches; pad8: a view of rows padded to a multiple of 8 elements (zeros), so
    the GEMMs reading it (the patch embedding's 147 columns) get 16-B aligned rows"""
    B, H, W, C = x.shape
    Ho = (H + 2 * pad - kh) // stride + 1
    Wo = (W + 2 * pad - kw) // stride + 1
    Kc = C * kh * kw
    ld = (Kc + 7) // 8 * 8 if pad8 else Kc
    buf = torch.empty(B * Ho * Wo, ld, device=x.device, dtype=x.dtype)
    call("s2h_im2col", dt(x), B, H, W, C, kh, kw, stride, pad, Ho, Wo, ld, ptr(x), ptr(buf), stream())
    return (buf[:, :Kc] if ld != Kc else buf), Ho, Wo


def dwconv(x, w, bias, pad):
    B, H, W, C = x.shape
    K = w.shape[-1]
    out = torch.empty_like(x)
    call("s2h_dwconv", dt(x), B, H, W, C, K, pad, ptr(x), ptr(w), ptr(bias), ptr(out), stream())
    return out


def convt2_scatter(Y, B, H, W, Co, bias=None, add=None, out=None):
    if out is None:
        out = torch.empty(B, 2 * H, 2 * W, Co, device=Y.device, dtype=Y.dtype)
    call("s2h_convt2", dt(Y), B, H, W, Co, ptr(Y), ptr(bias), ptr(add), ptr(out), 0, stream())
    return out


# S2H_CONVT_DIRECT=0: the scalar scatter + a separate (broadcast) add (A/B)
_CONVT_DIRECT = os.environ.get("S2H_CONVT_DIRECT", "1") == "1"


def convt2_direct():
    return _CONVT_DIRECT


def convt2_store(Y, B, H, W, Co, bias=None, add=None, out=None):
    """out = scatter(Y) + bias (+ add: [B or 1, 2H, 2W, Co], broadcast over B when it has one batch),
    vectorised, one rounding (s2h_convt2_store)"""
    if out is None:
        out = torch.empty(B, 2 * H, 2 * W, Co, device=Y.device, dtype=Y.dtype)
    bc = 0
    if add is not None:
        assert add.is_contiguous() and add.dtype == Y.dtype and add.shape[1:] == out.shape[1:]
        assert add.shape[0] in (1, B)
        bc = int(add.shape[0] == 1 and B > 1)
    call("s2h_convt2_store", dt(Y), B, H, W, Co, ptr(Y), ptr(bias), ptr(add), bc, ptr(out), stream())
    return out


def convt2_tail(Y, B, H, W, Co, bias, add, hyper, pre, post, masks):
    """pre = convt2_store(Y) + bias + add, post = gelu(pre), masks[b] = post[b] . hyper[b] (s2h_convt2_tail)"""
    bc = 0
    if add is not None:
        assert add.is_contiguous() and add.dtype == Y.dtype and add.shape[0] in (1, B)
        bc = int(add.shape[0] == 1 and B > 1)
    assert hyper.is_contiguous() and hyper.numel() == B * Co and pre.is_contiguous() and post.is_contiguous()
    call("s2h_convt2_tail", dt(Y), B, H, W, Co, ptr(Y), ptr(bias), ptr(add), bc, ptr(hyper), ptr(pre), ptr(post),
         ptr(masks), stream())
    return masks


def convt2_tail_enabled():
    return os.environ.get("S2H_CONVT_TAIL", "1") == "1"


def convt2_tail_k(Y, B, H, W, Co, bias, add, hyper, masks=None, pre=None, post=None):
    """masks[b, k] = gelu(convt2_store(Y) + bias + add)[b] . hyper[b, k] for the K = 4 mask tokens in one
    pass (s2h_convt2_tail_k; bf16, Co = 32); masks [B, K, 2H * 2W]; pre / post optional outputs"""
    K = hyper.shape[1]
    bc = 0
    if add is not None:
        assert add.is_contiguous() and add.dtype == Y.dtype and add.shape[0] in (1, B)
        assert add.numel() == add.shape[0] * 4 * H * W * Co
        bc = int(add.shape[0] == 1 and B > 1)
    assert Y.is_contiguous() and Y.numel() == B * H * W * 4 * Co
    assert hyper.is_contiguous() and hyper.dtype == Y.dtype and hyper.shape == (B, K, Co)
    if masks is None:
        masks = torch.empty(B, K, 4 * H * W, device=Y.device, dtype=Y.dtype)
    assert masks.is_contiguous() and masks.dtype == Y.dtype and masks.numel() == B * K * 4 * H * W
    for t in (pre, post):
        assert t is None or (t.is_contiguous() and t.dtype == Y.dtype and t.numel() == B * 4 * H * W * Co)
    _dev(Y, hyper, masks)
    call("s2h_convt2_tail_k", dt(Y), B, H, W, Co, K, ptr(Y), ptr(bias), ptr(add), bc, ptr(hyper), ptr(pre), ptr(post),
         ptr(masks), stream())
    return masks


def stability_counts(masks, delta, counts=None):
    """masks [B, P] (bf16 / fp32 rows, unit inner stride) -> int32 [B, 2]: per row the number of logits
    > delta and > -delta (s2h_stability_counts; the stability score's two areas, mask_decoder.py:247-257)"""
    B, P = masks.shape
    assert masks.stride(1) == 1 and (B == 1 or masks.stride(0) >= P)
    if counts is None:
        counts = torch.empty(B, 2, device=masks.device, dtype=torch.int32)
    assert counts.is_contiguous() and counts.dtype == torch.int32 and counts.shape == (B, 2)
    _dev(masks, counts)
    call("s2h_stability_counts", dt(masks), B, P, ptr(masks), masks.stride(0) if B > 1 else P, float(delta),
         ptr(counts), stream())
    return counts


def multimask_select(masks, iou, score, tokens, *, dynamic=False, counts=None, thresh=0.0, token_follows=False,
                     fill=0.0, want_candidates=False):
    """Output selection of the three-mask heads (s2h_multimask_select).  masks [B, K, P], iou [B, K] fp32,
    score [B] fp32, tokens [B, K, C] (rows of a larger token array allowed: unit inner strides).
    -> (idx int32 [B], low fp32 [B, P] gated by score > 0 else `fill`, iou fp32 [B], token [B, C],
    gated candidates 1..K-1 fp32 [B, K-1, P] or None)"""
    B, K, P = masks.shape
    C = tokens.shape[2]
    assert masks.is_contiguous() and tokens.dtype == masks.dtype and tokens.shape[:2] == (B, K)
    assert tokens.stride(2) == 1 and tokens.stride(1) == C and (B == 1 or tokens.stride(0) >= K * C)
    assert iou.is_contiguous() and iou.dtype == torch.float32 and iou.shape == (B, K)
    assert score.is_contiguous() and score.dtype == torch.float32 and score.numel() == B
    if dynamic:
        assert counts is not None and counts.is_contiguous() and counts.dtype == torch.int32 and counts.shape == (B, 2)
    dev = masks.device
    idx = torch.empty(B, device=dev, dtype=torch.int32)
    low = torch.empty(B, P, device=dev, dtype=torch.float32)
    iou_out = torch.empty(B, device=dev, dtype=torch.float32)
    tok_out = torch.empty(B, C, device=dev, dtype=masks.dtype)
    multi = torch.empty(B, K - 1, P, device=dev, dtype=torch.float32) if want_candidates else None
    _dev(masks, iou, score, tokens)
    call("s2h_multimask_select", dt(masks), B, K, P, C, ptr(masks), ptr(iou), ptr(counts) if dynamic else None,
         ptr(score), ptr(tokens), tokens.stride(0) if B > 1 else K * C, int(bool(dynamic)), int(bool(token_follows)),
         float(thresh), float(fill), ptr(idx), ptr(low), ptr(iou_out), ptr(tok_out), ptr(multi), stream())
    return idx, low, iou_out, tok_out, multi


def cc_label(scores, positive=True):
    """8-connected components of N images (s2h_cc_label).  scores [N, H, W] fp32 contiguous; foreground is
    scores > 0 (`positive`) or scores <= 0.  -> (labels, areas) int32 [N, H, W]: 0 off the foreground, else
    1 + the smallest in-image index of the pixel's component, and the component's pixel count."""
    assert scores.dim() == 3 and scores.dtype == torch.float32 and scores.is_contiguous()
    _dev(scores)
    N, H, W = scores.shape
    labels = torch.empty(N, H, W, device=scores.device, dtype=torch.int32)
    areas = torch.empty(N, H, W, device=scores.device, dtype=torch.int32)
    call("s2h_cc_label", N, H, W, ptr(scores), int(bool(positive)), ptr(labels), ptr(areas), stream())
    return labels, areas


def fill_holes(scores, max_area, out=None):
    """upstream fill_holes_in_mask_scores (s2h_fill_holes): background components of area <= max_area become
    0.1, then foreground components of area <= max_area of that result become -0.1; the rest is copied.
    scores [N, H, W] or [N, 1, H, W] fp32 contiguous -> the same shape.  The scratch (2 int32 per pixel)
    comes from the torch allocator, so the call can be captured in a HIP graph."""
    assert scores.dim() in (3, 4) and scores.dtype == torch.float32 and scores.is_contiguous()
    assert scores.dim() == 3 or scores.shape[1] == 1
    assert int(max_area) > 0, "max_area must be positive"
    if out is None:
        out = torch.empty_like(scores)
    assert out.shape == scores.shape and out.dtype == torch.float32 and out.is_contiguous()
    assert out.data_ptr() != scores.data_ptr() or scores.numel() == 0, "fill_holes does not run in place"
    _dev(scores, out)
    N, H, W = scores.shape[0], scores.shape[-2], scores.shape[-1]
    work = torch.empty(2 * N * H * W, device=scores.device, dtype=torch.int32)
    call("s2h_fill_holes", N, H, W, ptr(scores), int(max_area), ptr(out), ptr(work), stream())
    return out


# ------------------------------------------------------------------ prompts from ground truth (csrc/gtprompt.hip)
GP_STATS = 9        # int64 per kept component of s2h_cc_components (csrc/gtprompt.h)
GP_MAX_INDEX = 255  # kept components per image its uint8 index image can name
GP_MAX_REACH = 32   # a morphology window reaches at most this far to either side
GP_CHUNK = 4096     # pixels per counting block of s2h_mask_rank_select


def cc_label_u8(mask, positive=True):
    """cc_label on byte masks (s2h_cc_label_u8): mask [N, H, W] uint8 contiguous, foreground is != 0
    (`positive`) or == 0.  -> (labels, areas) int32 [N, H, W] as cc_label"""
    assert mask.dim() == 3 and mask.dtype == torch.uint8 and mask.is_contiguous()
    _dev(mask)
    N, H, W = mask.shape
    labels = torch.empty(N, H, W, device=mask.device, dtype=torch.int32)
    areas = torch.empty(N, H, W, device=mask.device, dtype=torch.int32)
    call("s2h_cc_label_u8", N, H, W, ptr(mask), int(bool(positive)), ptr(labels), ptr(areas), stream())
    return labels, areas


def rle_runs(counts_list, H, W):
    """COCO counts of A annotations of one H x W image -> (run_off int32 [A + 1], run_end int32 [sum of the
    run counts]) host numpy, what s2h_rle_decode reads; every annotation's counts must be >= 0 and sum to H W"""
    H, W = int(H), int(W)
    run_off, ends = [0], []
    for a, cnts in enumerate(counts_list):
        c = np.asarray(cnts, dtype=np.int64).reshape(-1)
        if c.size == 0 or (c < 0).any() or int(c.sum()) != H * W:
            raise ValueError(f"annotation {a}: RLE counts cover {int(c.sum())} pixels in {c.size} runs, "
                             f"the mask has {H * W}")
        ends.append(np.cumsum(c))
        run_off.append(run_off[-1] + c.size)
    run_end = np.concatenate(ends) if ends else np.zeros(0, np.int64)
    return np.asarray(run_off, np.int32), run_end.astype(np.int32)


def rle_decode(counts_list, H, W, device="cuda"):
    """COCO RLE counts (lists of run lengths, column-major, starting with zeros) of A annotations of one H x W
    image -> uint8 [A, H, W] on the device (s2h_rle_decode); only the run boundaries are uploaded"""
    run_off, run_end = rle_runs(counts_list, H, W)
    A = run_off.size - 1
    mask = torch.empty(A, int(H), int(W), device=device, dtype=torch.uint8)
    _dev(mask)
    if A == 0:
        return mask
    off_d = torch.from_numpy(run_off).to(mask.device)
    end_d = torch.from_numpy(run_end).to(mask.device)
    call("s2h_rle_decode", A, int(H), int(W), ptr(off_d), ptr(end_d), ptr(mask), stream())
    return mask


def rle_decode_runs(run_off, run_end, H, W):
    """rle_decode from run boundaries already on the device (int32, as rle_runs gives them) -> uint8 [A, H, W]"""
    for t in (run_off, run_end):
        assert t.dim() == 1 and t.dtype == torch.int32 and t.is_contiguous()
    _dev(run_off, run_end)
    A = run_off.numel() - 1
    mask = torch.empty(A, int(H), int(W), device=run_off.device, dtype=torch.uint8)
    if A > 0:
        call("s2h_rle_decode", A, int(H), int(W), ptr(run_off), ptr(run_end), ptr(mask), stream())
    return mask


PC_MAX_GROUP_ANNS = 1 << 12  # csrc/pair_counts.h: annotations per group and side


def rle_pair_counts(dt_groups, gt_groups, H, W, device="cuda"):
    """Offline scoring counts from the runs (s2h_rle_pair_counts).  dt_groups / gt_groups: G lists, one per
    (image, category) group of H x W images, of COCO counts (one list of run lengths per annotation) of the
    predicted resp. ground-truth side.  -> int64 [G, 4] on the device: |p & g|, |p | g|, |p|, |g| of the OR-ed
    sides.  Only the run boundaries are uploaded (rle_runs); no mask is decoded."""
    G = len(dt_groups)
    if len(gt_groups) != G:
        raise ValueError(f"{G} predicted groups, {len(gt_groups)} ground-truth groups")
    bufs = []
    for side, groups in (("predicted", dt_groups), ("ground-truth", gt_groups)):
        sizes = [len(g) for g in groups]
        if sizes and max(sizes) > PC_MAX_GROUP_ANNS:
            raise ValueError(f"a group has {max(sizes)} {side} annotations; at most {PC_MAX_GROUP_ANNS} are read")
        grp_off = np.concatenate([[0], np.cumsum(sizes, dtype=np.int64)]).astype(np.int32)
        run_off, run_end = rle_runs([c for g in groups for c in g], H, W)
        if run_end.size == 0:
            run_end = np.zeros(1, np.int32)  # never read: no annotation on this side
        bufs += [grp_off, run_off, run_end]
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("libsam2hip kernels run on the GPU only (device %s)" % dev)
    out = torch.empty(G, 4, device=dev, dtype=torch.int64)
    if G == 0:
        return out
    with torch.cuda.device(out.device):
        d = [torch.from_numpy(b).to(out.device) for b in bufs]
        call("s2h_rle_pair_counts", G, int(H), int(W), *[ptr(t) for t in d], ptr(out), stream())
    return out


# ------------------------------------------------------------------------------------------- clip loading
RS_BITS = 22       # csrc/resample_u8.h: Pillow's PRECISION_BITS
RS_MAX_TAPS = 64   # taps per output sample
RS_MAX_SIDE = 16384
RS_MAX_CATS = 64


def _pil_bilinear(x):
    x = -x if x < 0.0 else x
    return 1.0 - x if x < 1.0 else 0.0


def _pil_bicubic(x):
    a = -0.5
    x = -x if x < 0.0 else x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


_PIL_FILTERS = {"bilinear": (_pil_bilinear, 1.0), "bicubic": (_pil_bicubic, 2.0)}
_TAPS = {}


def resample_taps(in_size, out_size, filter="bilinear"):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc (libImaging/Resample.c) for one axis, in Python double
    arithmetic and in Pillow's order of operations -> (xmin int32 [out], cnt int32 [out], coef int32 [out, ksize])
    numpy: output sample o reads cnt[o] source samples from xmin[o], weighted by coef[o] / 2^22 (rows padded
    with zeros).  filter "bilinear" (support 1) or "bicubic" (support 2, a = -0.5).  Cached."""
    key = (int(in_size), int(out_size), filter)
    hit = _TAPS.get(key)
    if hit is not None:
        return hit
    in_size, out_size = key[0], key[1]
    if filter not in _PIL_FILTERS:
        raise ValueError(f"filter must be one of {sorted(_PIL_FILTERS)}, got {filter!r}")
    if in_size < 1 or out_size < 1:
        raise ValueError(f"sizes must be positive, got {in_size} -> {out_size}")
    f, support = _PIL_FILTERS[filter]
    scale = in_size / out_size
    fs = scale if scale >= 1.0 else 1.0
    sup = support * fs
    ksize = int(math.ceil(sup)) * 2 + 1
    ss = 1.0 / fs
    xmin = np.zeros(out_size, np.int32)
    cnt = np.zeros(out_size, np.int32)
    coef = np.zeros((out_size, ksize), np.int32)
    for o in range(out_size):
        center = (o + 0.5) * scale
        lo = max(int(center - sup + 0.5), 0)
        n = min(int(center + sup + 0.5), in_size) - lo
        w = [f((k + lo - center + 0.5) * ss) for k in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        for k in range(n):
            v = w[k] / ww if ww != 0.0 else w[k]
            coef[o, k] = int(-0.5 + v * (1 << RS_BITS)) if v < 0 else int(0.5 + v * (1 << RS_BITS))
        xmin[o], cnt[o] = lo, n
    for a in (xmin, cnt, coef):
        a.setflags(write=False)
    _TAPS[key] = (xmin, cnt, coef)
    return _TAPS[key]


_DEV_TABLES = {}


def _dev_table(key, device, make):
    """a small host-built int32 / fp32 table on `device`, uploaded once per key"""
    k = (key, str(device))
    t = _DEV_TABLES.get(k)
    if t is None:
        t = _DEV_TABLES[k] = tuple(torch.from_numpy(np.array(a, order="C")).to(device) for a in make())
    return t


def norm_lut(mean, std):
    """[3, 256] fp32: the normalised value of every byte, by the torch expressions the host loaders use
    (data/dataset.py load_image, predictor._load_frames): v.float() / 255, then (x - mean) / std"""
    x = torch.arange(256, dtype=torch.uint8).view(1, 256).expand(3, 256).contiguous().float().div_(255.0)
    m = torch.tensor(tuple(float(v) for v in mean)).view(3, 1)
    s = torch.tensor(tuple(float(v) for v in std)).view(3, 1)
    return ((x - m) / s).contiguous()


def resample_u8_norm(frames_u8, out_hw, crop_top_left=(0, 0), filter="bilinear", mean=(0.485, 0.456, 0.406),
                     std=(0.229, 0.224, 0.225), crop_hw=None, out=None):
    """PIL `Image.resize(out_hw, filter)`, `crop` and the normalisation of F uint8 RGB frames
    (s2h_resample_u8_norm): frames_u8 [F, H, W, 3] uint8 on the device -> [F, 3, ch, cw] fp32, bit for bit what
    the host computes.  out_hw = (h, w) of the resized image, crop_top_left = (top, left) and crop_hw = (ch, cw)
    of the window kept (default: the rest of the image)."""
    assert frames_u8.dim() == 4 and frames_u8.shape[-1] == 3 and frames_u8.dtype == torch.uint8
    assert frames_u8.is_contiguous()
    _dev(frames_u8)
    F, H, W, _ = frames_u8.shape
    nh, nw = (int(v) for v in out_hw)
    top, left = (int(v) for v in crop_top_left)
    ch, cw = (nh - top, nw - left) if crop_hw is None else (int(v) for v in crop_hw)
    if not (0 <= top and 0 <= left and ch >= 1 and cw >= 1 and top + ch <= nh and left + cw <= nw):
        raise ValueError(f"crop ({top}, {left}) + ({ch}, {cw}) is outside the resized image ({nh}, {nw})")
    xm, xc, xk = resample_taps(W, nw, filter)
    ym, yc, yk = resample_taps(H, nh, filter)
    kx, ky = xk.shape[1], yk.shape[1]
    if kx > RS_MAX_TAPS or ky > RS_MAX_TAPS:
        raise ValueError(f"{H} x {W} -> {nh} x {nw} ({filter}) needs {max(kx, ky)} taps, at most {RS_MAX_TAPS}")
    ymw, ycw = ym[top:top + ch], yc[top:top + ch]
    row0 = int(ymw.min())
    nrows = int((ymw + ycw).max()) - row0
    dev = frames_u8.device
    tx = _dev_table(("taps", W, nw, filter, left, cw), dev, lambda: (xm[left:left + cw], xc[left:left + cw],
                                                                      xk[left:left + cw]))
    ty = _dev_table(("taps", H, nh, filter, top, ch), dev, lambda: (ymw, ycw, yk[top:top + ch]))
    mean, std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
    lut, = _dev_table(("lut", mean, std), dev, lambda: (norm_lut(mean, std).numpy(),))
    if out is None:
        out = torch.empty(F, 3, ch, cw, device=dev, dtype=torch.float32)
    assert out.shape == (F, 3, ch, cw) and out.dtype == torch.float32 and out.is_contiguous() and out.device == dev
    scratch = torch.empty(max(1, F * nrows * cw * 3), device=dev, dtype=torch.uint8)
    call("s2h_resample_u8_norm", F, H, W, ptr(frames_u8), cw, kx, ptr(tx[0]), ptr(tx[1]), ptr(tx[2]), ch, ky,
         ptr(ty[0]), ptr(ty[1]), ptr(ty[2]), row0, nrows, ptr(lut), ptr(scratch), ptr(out), stream())
    return out


_NEAREST = {}


def nearest_maps(H, W, S):
    """(row_map int32 [S], col_map int32 [S]) numpy: the source row / column of every output row / column of
    data/dataset.py resize_mask on an H x W mask -- F.interpolate(mode="nearest") to the short-side-S size (its
    index rule, taken from torch itself on an arange), then the center crop.  Cached."""
    key = (int(H), int(W), int(S))
    hit = _NEAREST.get(key)
    if hit is None:
        from ..data.dataset import center_crop_box, resized_hw
        H, W, S = key
        nh, nw = resized_hw(H, W, S)
        top, left = center_crop_box(nh, nw, S, S)
        interp = torch.nn.functional.interpolate
        rows = interp(torch.arange(H, dtype=torch.float32)[None, None], size=nh, mode="nearest")[0, 0]
        cols = interp(torch.arange(W, dtype=torch.float32)[None, None], size=nw, mode="nearest")[0, 0]
        hit = (rows[top:top + S].to(torch.int32).numpy().copy(), cols[left:left + S].to(torch.int32).numpy().copy())
        for a in hit:
            a.setflags(write=False)
        _NEAREST[key] = hit
    return hit


def rle_catmasks(run_off, run_end, ann_cat, frame_off, H, W, row_map, col_map, num_categories, out=None):
    """category masks of F frames straight from COCO RLE run boundaries (s2h_rle_catmasks): run_off [A + 1] /
    run_end as ops.rle_runs gives them for the annotations of all frames back to back, ann_cat [A] the category
    index of each (outside [0, num_categories) = skipped), frame_off [F + 1] the annotations per frame (CSR),
    row_map [Sh] / col_map [Sw] the source row / column of every output row / column (ops.nearest_maps); all
    int32 on the device.  -> bool [F, num_categories, Sh, Sw]: what dataset.resize_mask(rle.decode(.)) OR-ed
    per category gives."""
    for t in (run_off, run_end, ann_cat, frame_off, row_map, col_map):
        assert t.dtype == torch.int32 and t.dim() == 1 and t.is_contiguous()
    _dev(run_off, run_end, ann_cat, frame_off, row_map, col_map)
    A, F, N = ann_cat.numel(), frame_off.numel() - 1, int(num_categories)
    assert run_off.numel() == A + 1 and F >= 0
    if not 0 <= N <= RS_MAX_CATS:
        raise ValueError(f"num_categories {N} is outside [0, {RS_MAX_CATS}]")
    Sh, Sw = row_map.numel(), col_map.numel()
    if out is None:
        out = torch.empty(F, N, Sh, Sw, device=frame_off.device, dtype=torch.bool)
    assert out.shape == (F, N, Sh, Sw) and out.dtype == torch.bool and out.is_contiguous()
    call("s2h_rle_catmasks", F, N, int(H), int(W), A, ptr(run_off), ptr(run_end), ptr(ann_cat), ptr(frame_off), Sh, Sw,
         ptr(row_map), ptr(col_map), ptr(out), stream())
    return out


def morph_rect(mask, op, y_win, x_win, out=None):
    """rectangular dilation (op "dilate" / 0) or erosion ("erode" / 1) of byte masks [N, H, W]
    (s2h_morph_rect): out(y, x) = OR / AND of mask(y + dy, x + dx) over dy in [y_win[0], y_win[1]] and dx in
    [x_win[0], x_win[1]] restricted to the image.  -32 <= lo <= 0 <= hi <= 32.  -> uint8 [N, H, W] of 0 / 1"""
    op = {"dilate": 0, "erode": 1}.get(op, op)
    assert op in (0, 1), "op is dilate (0) or erode (1)"
    assert mask.dim() == 3 and mask.dtype == torch.uint8 and mask.is_contiguous()
    (y_lo, y_hi), (x_lo, x_hi) = (int(v) for v in y_win), (int(v) for v in x_win)
    for lo, hi in ((y_lo, y_hi), (x_lo, x_hi)):
        if not (-GP_MAX_REACH <= lo <= 0 <= hi <= GP_MAX_REACH):
            raise ValueError(f"window ({lo}, {hi}) is outside -{GP_MAX_REACH} <= lo <= 0 <= hi <= {GP_MAX_REACH}")
    if out is None:
        out = torch.empty_like(mask)
    assert out.shape == mask.shape and out.dtype == torch.uint8 and out.is_contiguous()
    assert out.data_ptr() != mask.data_ptr() or mask.numel() == 0, "morph_rect does not run in place"
    _dev(mask, out)
    N, H, W = mask.shape
    work = torch.empty_like(mask)
    call("s2h_morph_rect", N, H, W, ptr(mask), op, y_lo, y_hi, x_lo, x_hi, ptr(out), ptr(work), stream())
    return out


def cc_components(labels, areas, min_area, grid=None, capacity=None):
    """the components of area >= min_area of images labelled by cc_label / cc_label_u8, per image in raster
    order of their first pixel (s2h_cc_components).  grid: uint8 [H, W] on the device or None.
    -> (hdr int32 [2 N + 2]: count and offset per image, total, status (1: an image has more than 255 kept
    components and `index` is unusable); stats int64 [capacity, 9]: root label, area, xmin, ymin, xmax, ymax,
    n_sel, sum x, sum y of the grid-selected pixels -- only the first min(total, capacity) rows are written;
    index uint8 [N, H, W]: 0 or the 1-based number of the pixel's kept component within its image).
    capacity None = 255 N, enough whenever the status is 0."""
    assert labels.dim() == 3 and labels.dtype == torch.int32 and labels.is_contiguous()
    assert areas.shape == labels.shape and areas.dtype == torch.int32 and areas.is_contiguous()
    _dev(labels, areas)
    N, H, W = labels.shape
    if grid is not None:
        assert grid.shape == (H, W) and grid.dtype == torch.uint8 and grid.is_contiguous()
        _dev(grid)
    capacity = GP_MAX_INDEX * N if capacity is None else int(capacity)
    dev = labels.device
    hdr = torch.empty(2 * N + 2, device=dev, dtype=torch.int32)
    stats = torch.empty(max(capacity, 1), GP_STATS, device=dev, dtype=torch.int64)[:capacity]
    index = torch.empty(N, H, W, device=dev, dtype=torch.uint8)
    work = torch.empty(max(1, N * H * W + N * ((H * W + 255) // 256)), device=dev, dtype=torch.int32)
    call("s2h_cc_components", N, H, W, ptr(labels), ptr(areas), int(min_area), ptr(grid), capacity, ptr(hdr),
         ptr(stats), ptr(index), ptr(work), stream())
    return hdr, stats, index


def mask_rank_select(q_img, q_label, q_neg, q_rank, labels, grid=None):
    """per query the q_rank-th pixel, row-major, of image q_img among those with (labels == q_label) != q_neg
    that lie on the grid (s2h_mask_rank_select).  The four query arrays: int32 [Q] on the device.
    -> (xy int32 [Q, 2] = (x, y), (-1, -1) when the rank is not below the count; count int32 [Q])"""
    assert labels.dim() == 3 and labels.dtype == torch.int32 and labels.is_contiguous()
    N, H, W = labels.shape
    Q = q_img.numel()
    for t in (q_img, q_label, q_neg, q_rank):
        assert t.dim() == 1 and t.numel() == Q and t.dtype == torch.int32 and t.is_contiguous()
    _dev(labels, q_img, q_label, q_neg, q_rank)
    if grid is not None:
        assert grid.shape == (H, W) and grid.dtype == torch.uint8 and grid.is_contiguous()
        _dev(grid)
    dev = labels.device
    xy = torch.empty(Q, 2, device=dev, dtype=torch.int32)
    count = torch.empty(Q, device=dev, dtype=torch.int32)
    work = torch.empty(max(1, Q * ((H * W + GP_CHUNK - 1) // GP_CHUNK)), device=dev, dtype=torch.int32)
    call("s2h_mask_rank_select", Q, ptr(q_img), ptr(q_label), ptr(q_neg), ptr(q_rank), N, H, W, ptr(labels),
         ptr(grid), ptr(xy), ptr(count), ptr(work), stream())
    return xy, count


# ------------------------------------------------------------------ correction clicks (csrc/clicks.hip)
CK_MAX_SIDE = 4092  # H, W of the three entries below (csrc/clicks.h): keeps D2 < 2^22


def _click_masks(gt, pred):
    assert gt.dim() == 3 and gt.dtype == torch.uint8 and gt.is_contiguous()
    _dev(gt)
    if pred is not None:
        assert pred.shape == gt.shape and pred.dtype == torch.uint8 and pred.is_contiguous()
        _dev(pred)
    B, H, W = gt.shape
    if not (1 <= H <= CK_MAX_SIDE and 1 <= W <= CK_MAX_SIDE):
        raise ValueError(f"masks of {H} x {W}: both sides must be in [1, {CK_MAX_SIDE}]")
    return B, H, W


def edt_sq(mask):
    """exact squared Euclidean distance transform of byte masks [N, H, W] (nonzero = set), the ring of pixels
    just outside the image counted as background (s2h_edt_sq): 0 where the mask is clear, else the smallest
    squared distance to a clear or outside pixel.  -> int32 [N, H, W]"""
    N, H, W = _click_masks(mask, None)
    dist2 = torch.empty(N, H, W, device=mask.device, dtype=torch.int32)
    work = torch.empty(max(1, N * H * W), device=mask.device, dtype=torch.int16)
    call("s2h_edt_sq", N, H, W, ptr(mask), ptr(dist2), ptr(work), stream())
    return dist2


def error_center_click(gt, pred=None):
    """per object the click at the centre of the larger error region (s2h_error_center_click): gt, pred uint8
    [B, H, W] (nonzero = set; pred None = the empty prediction).  -> (points fp32 [B, 2] = (x, y), labels int32
    [B]: 1 in the missed region, 0 in the wrongly predicted one, dmax int32 [B, 2]: the largest squared distance
    inside the missed and inside the wrongly predicted region)"""
    B, H, W = _click_masks(gt, pred)
    dev = gt.device
    points = torch.empty(B, 2, device=dev, dtype=torch.float32)
    labels = torch.empty(B, device=dev, dtype=torch.int32)
    dmax = torch.empty(B, 2, device=dev, dtype=torch.int32)
    nb = (H * W + 255) // 256
    work = torch.empty(max(1, 2 * B * nb + (B * H * W + 3) // 4), device=dev, dtype=torch.int64)
    call("s2h_error_center_click", B, H, W, ptr(gt), ptr(pred), ptr(points), ptr(labels), ptr(dmax), ptr(work),
         stream())
    return points, labels, dmax


def error_uniform_click(gt, pred, r):
    """per object P clicks drawn uniformly from the error regions, or from the background when there is no error
    (s2h_error_uniform_click): gt, pred as error_center_click; r int64 [B, P] draws in [0, 2^32): click (b, p) is
    the (r n) >> 32 -th of the n candidate pixels in row-major order.  -> (points fp32 [B, P, 2] = (x, y), labels
    int32 [B, P], count int32 [B, 2] = the candidates of label 0 and of label 1)"""
    B, H, W = _click_masks(gt, pred)
    assert r.dim() == 2 and r.shape[0] == B and r.dtype == torch.int64 and r.is_contiguous()
    _dev(r)
    P = r.shape[1]
    dev = gt.device
    points = torch.empty(B, P, 2, device=dev, dtype=torch.float32)
    labels = torch.empty(B, P, device=dev, dtype=torch.int32)
    count = torch.empty(B, 2, device=dev, dtype=torch.int32)
    work = torch.empty(max(1, 3 * B * ((H * W + GP_CHUNK - 1) // GP_CHUNK + 1)), device=dev, dtype=torch.int32)
    call("s2h_error_uniform_click", B, P, H, W, ptr(gt), ptr(pred), ptr(r), ptr(points), ptr(labels), ptr(count),
         ptr(work), stream())
    return points, labels, count


RLE_HDR = 8  # int32 per category of s2h_rle_transitions' header (csrc/rle_scan.h)


def rle_words(H, W):
    """uint64 words of one bit-packed H x W mask"""
    return (int(H) * int(W) + 63) // 64


SWEEP_MAX_K = 64  # cuts per s2h_mask_sweep call (csrc/sweep_hist.h)


def pack_mask_bits(masks):
    """bool [ncat, H, W] (numpy, or anything np.asarray takes) -> int64 [ncat, ceil(H W / 64)] numpy: the
    uint64 words of the column-major bit masks, bit j % 64 of word j // 64 = pixel (j % H, j // H) -- the
    layout s2h_mask_export writes and s2h_mask_sweep reads as ground truth.  Host numpy; unused tail bits 0."""
    m = np.asarray(masks).astype(bool)
    assert m.ndim == 3, "masks must be [ncat, H, W]"
    ncat, H, W = m.shape
    nw = rle_words(H, W)
    flat = np.zeros((ncat, nw * 64), dtype=bool)
    flat[:, :H * W] = m.transpose(0, 2, 1).reshape(ncat, H * W)
    words = np.packbits(flat.reshape(ncat, nw, 64), axis=2, bitorder="little").view("<u8").reshape(ncat, nw)
    return words.view(np.int64)


def mask_sweep(low, H, W, cat_off, cat_obj, ncat, cuts, gt_bits=None, non_overlap=False, hist=None):
    """the threshold sweep of one frame (s2h_mask_sweep).  low, cat_off, cat_obj, ncat, non_overlap as for
    mask_export; cuts [K] fp32 on the device, non-decreasing, 1 <= K <= 64 (eval/tune_threshold.py logit_cuts);
    gt_bits [ncat, ceil(H W / 64)] int64 on the device (pack_mask_bits) or None = all background.
    -> hist [ncat, 2, K + 1] int32 (overwritten): hist[c][g][b] = pixels of category c with ground-truth bit g
    whose merged value m has b = #{k : m >= cuts[k]}.  No scratch; capturable."""
    assert low.dim() == 3 and low.dtype == torch.float32 and low.is_contiguous()
    assert cat_off.dtype == torch.int32 and cat_obj.dtype == torch.int32 and cat_off.numel() == ncat + 1
    assert cat_off.is_contiguous() and cat_obj.is_contiguous()
    assert cuts.dim() == 1 and cuts.dtype == torch.float32 and cuts.is_contiguous()
    K = cuts.numel()
    assert 1 <= K <= SWEEP_MAX_K, f"1 <= K <= {SWEEP_MAX_K} cuts, got {K}"
    _dev(low, cat_off, cat_obj, cuts)
    N, hi, wi = low.shape
    H, W = int(H), int(W)
    if gt_bits is not None:
        assert gt_bits.shape == (ncat, rle_words(H, W)) and gt_bits.dtype == torch.int64 and gt_bits.is_contiguous()
        _dev(gt_bits)
    if hist is None:
        hist = torch.empty(ncat, 2, K + 1, device=low.device, dtype=torch.int32)
    assert hist.numel() == ncat * 2 * (K + 1) and hist.dtype == torch.int32 and hist.is_contiguous()
    _dev(hist)
    call("s2h_mask_sweep", N, hi, wi, H, W, ptr(low), ncat, ptr(cat_off), ptr(cat_obj), int(bool(non_overlap)),
         K, ptr(cuts), None if gt_bits is None else ptr(gt_bits), ptr(hist), stream())
    return hist


def mask_export(low, H, W, cat_off, cat_obj, ncat, non_overlap=False, bits=None, scores=None, cut=None, vmax=None):
    """category-merged bit masks and per-object scores of one frame (s2h_mask_export).  low [N, hi, wi] fp32
    contiguous low-res logits; cat_off [ncat + 1] / cat_obj int32: the object -> category CSR.
    -> (bits [ncat, ceil(H W / 64)] int64 holding the uint64 words of the column-major masks, bit j = pixel
    (j % H, j // H); scores [N] fp32 = mean sigmoid of the video-resolution logits).  The scratch comes from
    the torch allocator, so the call can be captured in a HIP graph.
    cut (a float; s2h_mask_export_cut): foreground is value >= cut instead of value > 0, and the result is
    (bits, scores, vmax [N] fp32 = each object's maximum video-resolution value)."""
    if cut is not None:
        return _mask_export_cut(low, H, W, cat_off, cat_obj, ncat, non_overlap, bits, scores, float(cut), vmax)
    assert vmax is None, "vmax is an output of mask_export(cut=...)"
    assert low.dim() == 3 and low.dtype == torch.float32 and low.is_contiguous()
    assert cat_off.dtype == torch.int32 and cat_obj.dtype == torch.int32 and cat_off.numel() == ncat + 1
    assert cat_off.is_contiguous() and cat_obj.is_contiguous()
    _dev(low, cat_off, cat_obj)
    N, hi, wi = low.shape
    H, W = int(H), int(W)
    nw = rle_words(H, W)
    if bits is None:
        bits = torch.empty(ncat, nw, device=low.device, dtype=torch.int64)
    if scores is None:
        scores = torch.empty(N, device=low.device, dtype=torch.float32)
    assert bits.shape == (ncat, nw) and bits.dtype == torch.int64 and bits.is_contiguous()
    assert scores.numel() == N and scores.dtype == torch.float32 and scores.is_contiguous()
    _dev(bits, scores)
    work = torch.empty(max(1, N * ((H * W + 255) // 256)), device=low.device, dtype=torch.float32)
    call("s2h_mask_export", N, hi, wi, H, W, ptr(low), ncat, ptr(cat_off), ptr(cat_obj), int(bool(non_overlap)),
         ptr(bits), ptr(scores), ptr(work), stream())
    return bits, scores


def _mask_export_cut(low, H, W, cat_off, cat_obj, ncat, non_overlap, bits, scores, cut, vmax):
    assert low.dim() == 3 and low.dtype == torch.float32 and low.is_contiguous()
    assert cat_off.dtype == torch.int32 and cat_obj.dtype == torch.int32 and cat_off.numel() == ncat + 1
    assert cat_off.is_contiguous() and cat_obj.is_contiguous()
    assert cut == cut, "cut must not be NaN"
    _dev(low, cat_off, cat_obj)
    N, hi, wi = low.shape
    H, W = int(H), int(W)
    nw = rle_words(H, W)
    if bits is None:
        bits = torch.empty(ncat, nw, device=low.device, dtype=torch.int64)
    if scores is None:
        scores = torch.empty(N, device=low.device, dtype=torch.float32)
    if vmax is None:
        vmax = torch.empty(N, device=low.device, dtype=torch.float32)
    assert bits.shape == (ncat, nw) and bits.dtype == torch.int64 and bits.is_contiguous()
    assert scores.numel() == N and scores.dtype == torch.float32 and scores.is_contiguous()
    assert vmax.numel() == N and vmax.dtype == torch.float32 and vmax.is_contiguous()
    _dev(bits, scores, vmax)
    work = torch.empty(max(1, 2 * N * ((H * W + 255) // 256)), device=low.device, dtype=torch.float32)
    call("s2h_mask_export_cut", N, hi, wi, H, W, ptr(low), ncat, ptr(cat_off), ptr(cat_obj), int(bool(non_overlap)),
         cut, ptr(bits), ptr(scores), ptr(vmax), ptr(work), stream())
    return bits, scores, vmax


def rle_transitions(bits, H, W, capacity=None, hdr=None, trans=None):
    """run boundaries, area and bounding box of bit-packed column-major masks (s2h_rle_transitions).
    bits [ncat, ceil(H W / 64)] int64.  -> (hdr [ncat, 8] int32 = n_trans, offset, area, xmin, ymin, xmax,
    ymax, total per category; trans [capacity] int32: category c's positions at offset[c] ..).  When
    total > capacity only the first `capacity` positions were written: call again with capacity >= total.
    capacity None = the worst case ncat * H * W."""
    assert bits.dim() == 2 and bits.dtype == torch.int64 and bits.is_contiguous()
    _dev(bits)
    ncat = bits.shape[0]
    H, W = int(H), int(W)
    nw = rle_words(H, W)
    assert bits.shape[1] == nw
    if trans is not None:
        capacity = trans.numel()
    elif capacity is None:
        capacity = ncat * H * W
    capacity = int(capacity)
    if hdr is None:
        hdr = torch.empty(ncat, RLE_HDR, device=bits.device, dtype=torch.int32)
    if trans is None:
        trans = torch.empty(capacity, device=bits.device, dtype=torch.int32)
    assert hdr.numel() == ncat * RLE_HDR and hdr.dtype == torch.int32 and hdr.is_contiguous()
    assert trans.dtype == torch.int32 and trans.is_contiguous()
    _dev(hdr, trans)
    work = torch.empty(max(1, 7 * ncat * ((nw + 255) // 256)), device=bits.device, dtype=torch.int32)
    call("s2h_rle_transitions", ncat, H, W, ptr(bits), capacity, ptr(hdr), ptr(trans), ptr(work), stream())
    return hdr, trans


# ---------------------------------------------------------------------- dataset preparation (csrc/dataprep.hip)
def label_hist(labels):
    """per frame the pixel count of every byte value (s2h_label_hist): labels [F, H, W] uint8 contiguous on the
    device -> int32 [F, 256]"""
    assert labels.dim() == 3 and labels.dtype == torch.uint8 and labels.is_contiguous()
    _dev(labels)
    F, H, W = labels.shape
    hist = torch.empty(F, 256, device=labels.device, dtype=torch.int32)
    call("s2h_label_hist", F, H, W, ptr(labels), ptr(hist), stream())
    return hist


def label_planes(labels, frame_off, plane_class):
    """row-major label bytes -> column-major bit words, one plane per (frame, class) (s2h_label_planes).
    labels [F, H, W] uint8; frame_off [F + 1] int32 (CSR, ascending from 0 to P): the planes of frame f are
    [frame_off[f], frame_off[f + 1]); plane_class [P] int32: plane p is labels[f] == plane_class[p], or
    labels[f] != 0 for -1; all on the device.  -> int64 [P, ceil(H W / 64)] holding the uint64 words in the
    layout of pack_mask_bits / mask_export, what rle_transitions reads."""
    assert labels.dim() == 3 and labels.dtype == torch.uint8 and labels.is_contiguous()
    for t in (frame_off, plane_class):
        assert t.dim() == 1 and t.dtype == torch.int32 and t.is_contiguous()
    _dev(labels, frame_off, plane_class)
    F, H, W = labels.shape
    P = plane_class.numel()
    assert frame_off.numel() == F + 1
    bits = torch.empty(P, rle_words(H, W), device=labels.device, dtype=torch.int64)
    if P:
        call("s2h_label_planes", F, H, W, ptr(labels), P, ptr(frame_off), ptr(plane_class), ptr(bits), stream())
    return bits


def mask_planes(mask_u8):
    """byte masks [N, H, W] uint8 (nonzero = set, e.g. what morph_rect writes) -> their bit words int64
    [N, ceil(H W / 64)]: label_planes with one plane of class -1 per mask"""
    N = mask_u8.shape[0]
    frame_off = torch.arange(N + 1, device=mask_u8.device, dtype=torch.int32)
    plane_class = torch.full((N,), -1, device=mask_u8.device, dtype=torch.int32)
    return label_planes(mask_u8, frame_off, plane_class)


# ---------------------------------------------------------------------- training visualisation (csrc/viz.hip)
def _viz_frames(t, inner):
    """(frame count, frame stride in elements) of a tensor whose frames are contiguous `inner`-shaped blocks"""
    assert t.dim() == 1 + len(inner) and tuple(t.shape[1:]) == tuple(inner), (tuple(t.shape), inner)
    assert t[0].is_contiguous() and (t.shape[0] == 1 or t.stride(0) >= 0)
    return t.shape[0], (t.stride(0) if t.shape[0] > 1 else 0)


def viz_pack(masks, out=None):
    """category words of [n, C, H, W] masks (s2h_viz_pack): bit c of word [f, y, x] = masks[f, c, y, x] > 0.5.
    uint8 / bool (set = non-zero) or fp32; each frame's [C, H, W] block contiguous, any frame stride >= 0 (a
    strided slice of a clip is read where it lies).  -> int64 [n, H, W] holding the uint64 words."""
    _dev(masks)
    if masks.dtype == torch.bool:
        masks = masks.view(torch.uint8)
    assert masks.dtype in (torch.uint8, torch.float32), masks.dtype
    n, stride = _viz_frames(masks, masks.shape[1:])
    _, C, H, W = masks.shape
    if out is None:
        out = torch.empty(n, H, W, device=masks.device, dtype=torch.int64)
    assert out.dtype == torch.int64 and out.is_contiguous() and out.numel() == n * H * W
    call("s2h_viz_pack", n, C, H, W, int(masks.dtype == torch.float32), ptr(masks), stride, ptr(out), stream())
    return out


def viz_compose(frames, frame0, gt_words, pred_words, palette, markers=None, prompt_words=None, out=None):
    """the 2 x 2 composites uint8 [n, 2H, 2W, 3] (s2h_viz_compose; the picture is csrc/viz_pixel.h).
    frames fp32 [n, 3, H, W] ImageNet-normalised or uint8 [n, H, W, 3], each frame contiguous, any frame stride;
    frame0 one frame of the same kind; gt_words / pred_words int64 [n, H, W] from viz_pack; palette uint8 [C, 3];
    markers int32 [M, 8] or None; prompt_words int64 [H, W] (mask prompts: no markers) or None."""
    _dev(frames, frame0, gt_words, pred_words, palette, markers, prompt_words, out)
    u8 = frames.dtype == torch.uint8
    assert u8 or frames.dtype == torch.float32
    n, H, W = gt_words.shape
    inner = (H, W, 3) if u8 else (3, H, W)
    nf, stride = _viz_frames(frames, inner)
    assert nf == n and frame0.dtype == frames.dtype and tuple(frame0.shape) == inner and frame0.is_contiguous()
    for w in (gt_words, pred_words):
        assert w.dtype == torch.int64 and w.is_contiguous() and tuple(w.shape) == (n, H, W)
    assert palette.dtype == torch.uint8 and palette.dim() == 2 and palette.shape[1] == 3 and palette.is_contiguous()
    M = 0
    if markers is not None and markers.numel():
        assert markers.dtype == torch.int32 and markers.dim() == 2 and markers.shape[1] == 8 and markers.is_contiguous()
        M = markers.shape[0]
    if prompt_words is not None:
        assert prompt_words.dtype == torch.int64 and prompt_words.is_contiguous() and prompt_words.numel() == H * W
    if out is None:
        out = torch.empty(n, 2 * H, 2 * W, 3, device=frames.device, dtype=torch.uint8)
    assert out.dtype == torch.uint8 and out.is_contiguous() and out.numel() == n * 12 * H * W
    call("s2h_viz_compose", n, palette.shape[0], H, W, int(u8), ptr(frames), stride, ptr(frame0), ptr(gt_words),
         ptr(pred_words), ptr(prompt_words), ptr(palette), M, ptr(markers) if M else None, ptr(out), stream())
    return out


def convt2_gather(dout, B, H, W, Co, dY=None):
    if dY is None:
        dY = torch.empty(B * H * W, 4 * Co, device=dout.device, dtype=dout.dtype)
    call("s2h_convt2", dt(dout), B, H, W, Co, ptr(dout), None, None, ptr(dY), 1, stream())
    return dY


def row_gate(x, gate, fill, out=None, backward=False):
    rows = x.shape[0]
    if out is None:
        out = torch.empty_like(x)
    call("s2h_row_gate", dt(x), rows, x.numel() // rows, ptr(x), ptr(gate), float(fill), ptr(out), int(backward),
         stream())
    return out


def row_gate_cast(x, gate, fill, dtype, out=None, backward=False, gate_out=None):
    """row_gate with the output in `dtype` (s2h_row_gate_cast); gate_out: the gate copied beside it"""
    rows = x.shape[0]
    if out is None:
        out = torch.empty(x.shape, device=x.device, dtype=dtype)
    call("s2h_row_gate_cast", dt(x), dt(out), rows, x.numel() // rows, ptr(x), ptr(gate), float(fill), ptr(out),
         int(backward), ptr(gate_out), stream())
    return out


def gate_mix(x, gate, vec, scale_x=False, out=None):
    rows = x.shape[0]
    if out is None:
        out = torch.empty_like(x)
    call("s2h_gate_mix", dt(x), rows, x.numel() // rows, ptr(x), ptr(gate), ptr(vec), vec.numel(), int(scale_x),
         ptr(out), stream())
    return out


# ------------------------------------------------------------------ loss
NSTAT = 6


def mask_stats(x, tgt, inv_temp=1.0, stats=None):
    """x [N, P] f32 logits, tgt [N, P] uint8/bool (or None) -> stats [N, 6] f32"""
    N, P = x.shape
    if stats is None:
        stats = torch.empty(N, NSTAT, device=x.device, dtype=torch.float32)
    call("s2h_mask_stats", N, P, ptr(x), x.stride(0), ptr(tgt), tgt.stride(0) if tgt is not None else 0,
         float(inv_temp), ptr(stats), stream())
    return stats


def mask_loss_finalize(stats, pred_iou, valid, P, weights, gscale, losses, coef):
    N = stats.shape[0]
    call("s2h_mask_loss_finalize", N, P, ptr(stats), ptr(pred_iou), ptr(valid), float(weights[0]),
         float(weights[1]), float(weights[2]), float(gscale), ptr(losses), ptr(coef), stream())


def mask_loss_bwd(x, tgt, coef, inv_temp, dx, gtot=None, dious=None):
    N, P = x.shape
    call("s2h_mask_loss_bwd", N, P, ptr(x), x.stride(0), ptr(tgt), tgt.stride(0), float(inv_temp), ptr(coef),
         ptr(dx), dx.stride(0), ptr(gtot), ptr(dious), stream())
    return dx


def bce_stats(x, tgt, inv_temp=1.0, pos_weight=None):
    """x [N, P] f32 logits, tgt [N, P] uint8 -> stats [N, 2] (bce sum, target sum)"""
    N, P = x.shape
    stats = torch.empty(N, 2, device=x.device, dtype=torch.float32)
    call("s2h_bce_stats", N, P, ptr(x), x.stride(0), ptr(tgt), tgt.stride(0), float(inv_temp), ptr(pos_weight),
         ptr(stats), stream())
    return stats


def bce_finalize(stats, P, reduction, frame_scale, losses, coef):
    call("s2h_bce_finalize", stats.shape[0], P, ptr(stats), int(reduction), float(frame_scale), ptr(losses),
         ptr(coef), stream())


def bce_bwd(x, tgt, inv_temp, pos_weight, coef, dx, gtot=None):
    N, P = x.shape
    call("s2h_bce_bwd", N, P, ptr(x), x.stride(0), ptr(tgt), tgt.stride(0), float(inv_temp), ptr(pos_weight),
         ptr(coef), ptr(gtot), ptr(dx), dx.stride(0), stream())
    return dx


def group_max(x, cat_off, cat_obj, ncat, out, arg):
    P = x.shape[1]
    call("s2h_group_max_fwd", ncat, P, ptr(cat_off), ptr(cat_obj), ptr(x), x.stride(0), ptr(out), out.stride(0),
         ptr(arg), stream())
    return out


def group_max_bwd(dy, obj_cat, arg, dx):
    O, P = dx.shape
    call("s2h_group_max_bwd", O, P, ptr(obj_cat), ptr(arg), ptr(dy), dy.stride(0), ptr(dx), dx.stride(0), stream())
    return dx


def group_wavg(x, stats, cat_off, cat_obj, ncat, out):
    K = x.shape[1]
    call("s2h_group_wavg_fwd", ncat, K, ptr(cat_off), ptr(cat_obj), ptr(stats), ptr(x), ptr(out), stream())
    return out


def group_wavg_bwd(x, y, dy, stats, obj_cat, cat_off, dx, dw):
    O, K = x.shape
    call("s2h_group_wavg_bwd", O, K, ptr(obj_cat), ptr(cat_off), ptr(stats), ptr(x), ptr(y), ptr(dy), ptr(dx),
         ptr(dw), stream())


def sigmoid_grad_axpy(x, coef, dx):
    R, P = x.shape
    call("s2h_sigmoid_grad_axpy", R, P, ptr(x), x.stride(0), ptr(coef), ptr(dx), dx.stride(0), stream())
    return dx


# ------------------------------------------------------------- optimizer
def grad_norm(g, max_norm, ws, out, grad_scale=1.0):
    """out[0] = ||grad_scale*g||, out[1] = grad_scale * clip coefficient (device scalars)"""
    call("s2h_grad_norm", g.numel(), ptr(g), ptr(ws), float(max_norm), float(grad_scale), ptr(out), stream())
    return out


def adamw(p, g, m, v, clip, lr, beta1, beta2, eps, wd, step, shadow=None):
    call("s2h_adamw", p.numel(), ptr(p), ptr(g), ptr(m), ptr(v), ptr(clip), float(lr), float(beta1), float(beta2),
         float(eps), float(wd), int(step), ptr(shadow), stream())


def swa_update(avg, p, n_averaged):
    """avg = p (n_averaged == 0) or avg + (p - avg) / (n_averaged + 1), in place (s2h_swa_update): fp32, an
    IEEE division -- Lightning's StochasticWeightAveraging.avg_fn with its device-tensor divisor"""
    _dev(avg, p)
    assert avg.dtype == p.dtype == torch.float32 and avg.numel() == p.numel()
    assert avg.is_contiguous() and p.is_contiguous() and int(n_averaged) >= 0
    call("s2h_swa_update", avg.numel(), ptr(avg), ptr(p), int(n_averaged), stream())
    return avg


def swa_apply(avg, p, shadow=None):
    """p = avg and shadow = bf16(avg) (the rounding of adamw / cast), written in place (s2h_swa_apply)"""
    _dev(avg, p, shadow)
    assert avg.dtype == p.dtype == torch.float32 and avg.numel() == p.numel()
    assert avg.is_contiguous() and p.is_contiguous()
    assert shadow is None or (shadow.dtype == torch.bfloat16 and shadow.numel() == p.numel() and shadow.is_contiguous())
    call("s2h_swa_apply", p.numel(), ptr(avg), ptr(p), ptr(shadow), stream())
    return p


def pos_embed(Y, win, h, w, out):
    """out [h, w, C] = Y [C, h, w] + tile(win [C, ws, ws])"""
    C = Y.shape[0]
    ws = win.shape[-1]
    call("s2h_pos_embed", dt(out), C, h, w, ws, ptr(Y), ptr(win.contiguous()), ptr(out), stream())
    return out


def pos_embed_bwd(dout, dY, dwin, ws):
    h, w, C = dout.shape
    call("s2h_pos_embed_bwd", dt(dout), C, h, w, ws, ptr(dout), ptr(dY), ptr(dwin), stream())


def point_embed(pe, labels, table, out, labels_out=None):
    R, D = pe.shape
    assert labels_out is None or (labels_out.dtype == torch.int32 and labels_out.numel() == R)
    call("s2h_point_embed", dt(out), R, D, ptr(pe), ptr(labels), ptr(table), ptr(out), ptr(labels_out), stream())
    return out


def point_embed_bwd(labels, dout, dtable):
    R, D = dout.shape
    call("s2h_point_embed_bwd", dt(dout), R, D, ptr(labels), ptr(dout), ptr(dtable), stream())


def point_embed_bwd_rows(labels, dout, rows):
    """point_embed_bwd into 5 separate fp32 [D] rows (each accumulated in row order)"""
    import ctypes
    R, D = dout.shape
    assert len(rows) == 5 and all(r.dtype == torch.float32 and r.numel() == D and r.is_contiguous() for r in rows)
    arr = (ctypes.c_void_p * 5)(*[ptr(r) for r in rows])
    call("s2h_point_embed_bwd_rows", dt(dout), R, D, ptr(labels), ptr(dout), ctypes.addressof(arr), stream())


def version():
    from ._lib import lib
    return lib().s2h_version()


_ = math


def mask_down_stage(x, w, bias, gamma, beta, eps, *, logits=None, scale=1.0, shift=0.0, dtype=None):
    """Fused MaskDownSampler stage: GELU(LN2d(conv3x3/2(x))) on NHWC x [O, H, W, cin];
    or, with `logits` ([O, H, W] fp32), on sigmoid(logits) * scale + shift (cin = 1)."""
    cout, cin = w.shape[0], w.shape[1]
    assert tuple(w.shape[2:]) == (3, 3) and w.dtype == torch.float32 and w.is_contiguous()
    src = logits if logits is not None else x
    assert src.is_contiguous()
    O, H, W = src.shape[0], src.shape[1], src.shape[2]
    if logits is not None:
        assert logits.dtype == torch.float32 and cin == 1 and dtype is not None
    else:
        assert x.shape[-1] == cin
        dtype = x.dtype
    y = torch.empty(O, (H + 1) // 2, (W + 1) // 2, cout, device=src.device, dtype=dtype)
    call("s2h_mask_down_stage", BF16 if dtype == torch.bfloat16 else F32, O, H, W, cin, cout, ptr(src),
         int(logits is not None), float(scale), float(shift), ptr(w), ptr(bias), ptr(gamma), ptr(beta), float(eps),
         ptr(y), stream())
    return y


def mask_eval_counts(logits, tgt):
    """[N, 4] int64 counts (|pred & gt|, |pred | gt|, |pred|, |gt|) per category, pred = logits > 0.
    logits [N, ...] fp32, tgt [N, ...] bool/uint8 of the same pixel count."""
    N = logits.shape[0]
    x = logits.reshape(N, -1)
    t = tgt.reshape(N, -1)
    if t.dtype == torch.bool:
        t = t.view(torch.uint8)
    assert x.dtype == torch.float32 and t.dtype == torch.uint8 and x.shape == t.shape
    assert x.stride(-1) == 1 and t.stride(-1) == 1
    out = torch.empty(N, 4, device=x.device, dtype=torch.int64)
    call("s2h_mask_eval_counts", N, x.shape[1], ptr(x), x.stride(0), ptr(t), t.stride(0), ptr(out), stream())
    return out
