"""Per-element contract of the GEMM epilogues (csrc/gemm_epi.h: every bf16 tiling, the MX-fp8 kernel,
the tiny split-K reducer; csrc/gemm.hip: the fp32 kernel) against an fp64 model.

The accumulator is made exact -- integer operands in {-2..2}, K <= 136 (1024 for the tiny split-K
case), so |acc| <= 4096 is an exact fp32 integer for any tiling and K order -- and every optional term
has magnitude in [0.5, 2]: a term missing from, or misapplied to, ONE element is an error >= 0.5
against a bound of a few hundredths.  The model applies the kernels' order, rounding only where the
kernel stores:

  v = alpha*acc + bias[col | row];  X = round(v) (aux_mode 1);  v = act(v)  or  v *= act'(X) (aux_mode 2);
  v *= cscale[col];  dropout (oracle/dropout_oracle.py);  + R;  + beta*C_old;  round to dt_c.

Bound per element, S = the sum of the absolute values of the terms of the final sum:
  fp32 output |got - ref| <= 2^-20 S (<= 8 fp32 roundings + the 1.2e-7 error of the erfc fit),
  bf16 output 2^-8 |ref| + 2^-20 S (one output rounding, one bit wider for ties after the fp32 error);
the stored X likewise.  The first term of the final sum is itself computed from the sum alpha*acc + bias
(and, for GELU', Phi(X) + X phi(X)), whose fp32 rounding error is relative to ITS terms' magnitudes and
survives a cancellation: its contribution to S is max(|term|, L (|alpha*acc| + |bias|) |cscale| / (1 - p))
with L the activation's Lipschitz constant (1, 1, 1.13, 0.25), or for aux_mode 2
(|alpha*acc| + |bias|) * sum|terms of act'(X)|.
Padding between rows / batches and around misaligned bases holds a sentinel that must survive."""
import math
import zlib

import numpy as np
import pytest
import torch

from oracle import dropout_oracle as dr
from oracle import mx8_oracle as mx

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
SENT = -9.0  # fills every element no launch may write (exact in bf16)
SEED = 2**40 + 77
NONE, RELU, GELU, SIGM = 0, 1, 2, 3
LIP = {NONE: 1.0, RELU: 1.0, GELU: 1.13, SIGM: 0.25}

# option cases: one list, not a product
OPTIONS = {
    "bias0": dict(),
    "bias1": dict(bias=1),
    "bias2": dict(bias=2),
    "none+pre": dict(bias=1, aux=1, act=NONE),
    "relu+pre": dict(bias=1, aux=1, act=RELU),
    "gelu+pre": dict(bias=2, aux=1, act=GELU),
    "sigmoid+pre": dict(bias=1, aux=1, act=SIGM),
    "relu'": dict(aux=2, act=RELU),
    "gelu'": dict(aux=2, act=GELU),
    "sigmoid'": dict(aux=2, act=SIGM, bias=1),
    "cscale": dict(bias=1, cscale=True),
    "drop+R": dict(bias=1, p=0.1, R=True, idx0=2**33 + 5),
    "alpha": dict(bias=1, alpha=0.75),
    "beta1": dict(beta=1.0),
    "beta.5": dict(bias=1, beta=0.5),
    "all": dict(alpha=0.75, bias=2, act=GELU, aux=1, cscale=True, p=0.1, R=True, beta=0.5, idx0=6),
    "all'": dict(alpha=0.75, bias=1, act=SIGM, aux=2, cscale=True, p=0.1, R=True, beta=1.0, idx0=7),
}

# name: batch, M, N, K, ldc, ldr, ldx, base offset (elements past a 16-B boundary), batch-stride padding
SHAPES = {
    "n64-8col": (1, 70, 64, 40, 64, 64, 64, 0, 0),          # every wave's column block whole: 8-column path
    "n72-8col+ragged": (1, 70, 72, 136, 72, 72, 72, 0, 0),  # 8-column blocks + a ragged block on the 4-column path
    "n102-ldc104": (1, 130, 102, 40, 104, 104, 104, 0, 0),  # last group has 2 valid columns
    "n101-scalar": (1, 70, 101, 136, 101, 101, 101, 0, 0),  # scalar everywhere
    "ldr+8-ldx+4": (1, 70, 72, 40, 72, 80, 76, 0, 0),       # X falls back to 8-B accesses
    "base+1": (1, 70, 72, 40, 72, 72, 72, 1, 0),            # all vector flags off
    "base+4": (1, 70, 72, 136, 72, 72, 72, 4, 0),           # vecC on, vec8 off (bf16)
    "batch3-padded": (3, 70, 64, 40, 72, 72, 72, 0, 8),     # 8-column path with ldc != N, padded batch strides
}


@pytest.fixture(scope="module")
def ops():
    from sam2_video.kernels import ops as o
    return o


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _signed(shape, g, dtype):
    """values of magnitude in [0.5, 2] and random sign, exact in `dtype`"""
    v = (0.5 + 1.5 * torch.rand(shape, generator=g)) * (torch.randint(0, 2, shape, generator=g) * 2 - 1)
    return v.to(dtype)


class Strided:
    """a [batch, M, N] view (strides sb, ld, 1) `off` elements into a sentinel-filled flat device buffer"""

    def __init__(self, values, ld, off, pad):
        batch, M, N = values.shape
        self.sb = M * ld + pad
        n = off + batch * self.sb + 16
        self.flat = torch.full((n,), SENT, device=DEV, dtype=values.dtype)
        self.view = torch.as_strided(self.flat, (batch, M, N), (self.sb, ld, 1), off)
        self.view.copy_(values)
        self.ld = ld
        self.valid = torch.zeros(n, dtype=torch.bool, device=DEV)
        torch.as_strided(self.valid, (batch, M, N), (self.sb, ld, 1), off).fill_(True)

    def padding_intact(self):
        return bool((self.flat[~self.valid] == SENT).all())


_OPERANDS = {}


def _operands(batch, M, N, K, lo=-2, hi=2):
    """integer operands A [batch, M, K], B [batch, N, K] (fp32 CPU) and their exact product (fp64)"""
    key = (batch, M, N, K, lo, hi)
    if key not in _OPERANDS:
        g = _gen("ab", *key)
        a = torch.randint(lo, hi + 1, (batch, M, K), generator=g).float()
        b = torch.randint(lo, hi + 1, (batch, N, K), generator=g).float()
        acc = a.double() @ b.double().transpose(1, 2)
        assert acc.abs().max() <= 4096
        _OPERANDS[key] = (a, b, acc)
    return _OPERANDS[key]


def _act(v, act):
    if act == RELU:
        return v.clamp(min=0)
    if act == GELU:
        return 0.5 * v * (1 + torch.erf(v / math.sqrt(2)))
    if act == SIGM:
        return 1 / (1 + torch.exp(-v))
    return v


def _act_grad(x, act):
    """(act'(x), sum of the absolute values of its terms)"""
    if act == RELU:
        g = (x > 0).double()
        return g, g
    if act == GELU:
        cdf = 0.5 * (1 + torch.erf(x / math.sqrt(2)))
        xpdf = x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)
        return cdf + xpdf, cdf + xpdf.abs()
    if act == SIGM:
        s = 1 / (1 + torch.exp(-x))
        return s * (1 - s), s * (1 - s)
    one = torch.ones_like(x)
    return one, one


def _model(acc, o, bias, cscale, xin, R, cold, batch, M, N):
    """fp64 model -> (C reference, S, X reference or None, |alpha acc| + |bias|)"""
    alpha, beta, p = o.get("alpha", 1.0), o.get("beta", 0.0), o.get("p", 0.0)
    act, aux = o.get("act", NONE), o.get("aux", 0)
    v = alpha * acc
    spre = v.abs()
    if o.get("bias", 0) == 1:
        v = v + bias.double()[None, None, :]
        spre = spre + bias.double().abs()[None, None, :]
    elif o.get("bias", 0) == 2:
        v = v + bias.double()[None, :, None]
        spre = spre + bias.double().abs()[None, :, None]
    xref = v.clone() if aux == 1 else None
    if aux == 2:
        gr, gabs = _act_grad(xin.double(), act)
        t, tmag = v * gr, spre * gabs
    else:
        t = _act(v, act)
        tmag = torch.maximum(t.abs(), LIP[act] * spre)
    if cscale is not None:
        t = t * cscale.double()[None, None, :]
        tmag = tmag * cscale.double().abs()[None, None, :]
    if p > 0:
        idx = np.uint64(o["idx0"]) + np.arange(batch * M * N, dtype=np.uint64)  # drop_idx0 + (b*M + m)*N + n
        keep = torch.from_numpy(dr.keep(SEED, idx, p).reshape(batch, M, N)).double()
        inv = 1.0 / (1.0 - float(np.float32(p)))
        t, tmag = t * keep * inv, tmag * keep * inv
    S = tmag
    if R is not None:
        t, S = t + R.double(), S + R.double().abs()
    if beta != 0:
        t, S = t + beta * cold.double(), S + (beta * cold.double()).abs()
    return t, S, xref, spre


def _assert_within(got, ref, S, dtype, what):
    err = (got.double().cpu() - ref).abs()
    bound = 2.0 ** -20 * S + (2.0 ** -8 * ref.abs() if dtype == BF else 0.0)
    bad = err > bound
    if bad.any():
        i = tuple(int(x) for x in torch.nonzero(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements outside the bound; first at {i}: "
                             f"got {float(got[i]):.7g} want {float(ref[i]):.7g} bound {float(bound[i]):.3g}; "
                             f"max err/bound {float((err / bound.clamp(min=1e-300)).max()):.3g}")


def _run_option(name, o, shape, ab_dtype, c_dtype, launch, K=None, lo=-2, hi=2, has_cscale=True):
    """one option case on one shape: build the inputs, launch, compare C (and X) with the model"""
    batch, M, N, K0, ldc, ldr, ldx, off, pad = shape
    K = K or K0
    rx_dtype = ab_dtype if ab_dtype != "mx8" else BF
    a, b, acc = _operands(batch, M, N, K, lo, hi)
    g = _gen(name, *shape)
    aux, bmode = o.get("aux", 0), o.get("bias", 0)
    bias = None if not bmode else _signed((N if bmode == 1 else M,), g, F32)
    cscale = _signed((N,), g, F32) if o.get("cscale") and has_cscale else None
    R = _signed((batch, M, N), g, rx_dtype) if o.get("R") else None
    xin = _signed((batch, M, N), g, rx_dtype) if aux == 2 else None
    cold = _signed((batch, M, N), g, c_dtype)
    Cb = Strided(cold.to(DEV), ldc, off, pad)
    Rb = Strided(R.to(DEV), ldr, off, pad) if R is not None else None
    Xb = None
    if aux:
        Xb = Strided((xin if aux == 2 else torch.full((batch, M, N), SENT, dtype=rx_dtype)).to(DEV), ldx, off, pad)
    launch(a, b, Cb, Rb, Xb, o, None if bias is None else bias.to(DEV), None if cscale is None else cscale.to(DEV),
           aux_layout_nn=aux == 2)
    torch.cuda.synchronize()
    ref, S, xref, spre = _model(acc, o, bias, cscale, xin, R, cold, batch, M, N)
    _assert_within(Cb.view, ref, S, c_dtype, f"{name}: C")
    assert Cb.padding_intact(), f"{name}: padding of C overwritten"
    if aux == 1:
        _assert_within(Xb.view, xref, spre, rx_dtype, f"{name}: X")
    if aux:
        assert Xb.padding_intact(), f"{name}: padding of X overwritten"
        if aux == 2:
            assert torch.equal(Xb.view.cpu(), xin), f"{name}: X modified by aux_mode 2"


def _gemm_launcher(ops, ab_dtype):
    def launch(a, b, Cb, Rb, Xb, o, bias, cscale, aux_layout_nn):
        batch, M, K = a.shape
        N = b.shape[1]
        ad = a.to(DEV).to(ab_dtype)
        if aux_layout_nn:  # the dgrad layout: B [K, N], N-contiguous
            bd = b.transpose(1, 2).contiguous().to(DEV).to(ab_dtype)
            ldb = dict(ldb_k=N, ldb_n=1)
        else:
            bd = b.to(DEV).to(ab_dtype)
            ldb = dict(ldb_k=1, ldb_n=K)
        ops.gemm(ad, bd, Cb.view, M=M, N=N, K=K, lda_m=K, lda_k=1, ldc=Cb.ld, batch=batch, sA=M * K, sB=N * K,
                 sC=Cb.sb, bias=bias, bias_mode=o.get("bias", 0) or 1, residual=None if Rb is None else Rb.view,
                 ldr=0 if Rb is None else Rb.ld, sR=0 if Rb is None else Rb.sb, aux=None if Xb is None else Xb.view,
                 ldx=0 if Xb is None else Xb.ld, sX=0 if Xb is None else Xb.sb,
                 aux_mode=o.get("aux", 0),
                 cscale=cscale, drop_p=o.get("p", 0.0), seed=SEED, drop_idx0=o.get("idx0", 0), alpha=o.get("alpha", 1.0),
                 beta=o.get("beta", 0.0), act=o.get("act", NONE), **ldb)
    return launch


def _run_all(shape, ab_dtype, c_dtype, launch, **kw):
    failures = []
    for name, o in OPTIONS.items():
        try:
            _run_option(name, o, shape, ab_dtype, c_dtype, launch, **kw)
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, f"{len(failures)} option case(s) failed:\n" + "\n".join(failures)


@pytest.mark.parametrize("shape", list(SHAPES), ids=list(SHAPES))
@pytest.mark.parametrize("cfg", [0, 1, 5, 20, 25, 26, 29, -1])
def test_bf16_epilogue(ops, cfg, shape):
    """every option case on every shape / alignment, per forced bf16 tiling (a tiling that refuses a
    shape falls back inside the library, as test_gemm_every_tiling relies on)"""
    from sam2_video.kernels._lib import lib
    prev = lib().s2h_gemm_config(cfg)
    try:
        _run_all(SHAPES[shape], BF, BF, _gemm_launcher(ops, BF))
    finally:
        lib().s2h_gemm_config(prev)


@pytest.mark.parametrize("shape", list(SHAPES), ids=list(SHAPES))
def test_bf16_operands_fp32_output_epilogue(ops, shape):
    """bf16 A / B with an fp32 C: R and X stay bf16 (the A / B element type)"""
    _run_all(SHAPES[shape], BF, F32, _gemm_launcher(ops, BF))


@pytest.mark.parametrize("shape", list(SHAPES), ids=list(SHAPES))
@pytest.mark.parametrize("small", [1, 0])
def test_fp32_epilogue(ops, small, shape):
    """the fp32 kernel's own epilogue on its 32 x 32 and 64 x 64 tiles"""
    from sam2_video.kernels._lib import lib
    prev = lib().s2h_gemm_f32_small(small)
    try:
        _run_all(SHAPES[shape], F32, F32, _gemm_launcher(ops, F32))
    finally:
        lib().s2h_gemm_f32_small(prev)


def test_fp32_epilogue_128_tiles(ops):
    """batch 128 of 130 x 130 (K = 8): 512 tiles of 128 x 128, the big-tile rule, 2 rows / columns in
    the ragged tiles"""
    shape = (128, 130, 130, 8, 130, 130, 130, 0, 0)
    launch = _gemm_launcher(ops, F32)
    for name in ("bias2", "all", "all'"):
        _run_option(name, OPTIONS[name], shape, F32, F32, launch)


@pytest.mark.parametrize("shape", ["n72-8col+ragged", "n101-scalar"])
def test_tiny_splitk_epilogue(ops, shape):
    """the tiny split-K reducer's epilogue4 call (M <= 128, K = 1024, one fp32 split launch + the reduce)"""
    from sam2_video.kernels._lib import lib
    ws = ops.wgrad_workspace(DEV)
    prev = lib().s2h_gemm_tiny_splitk(1)
    try:
        # (aux_mode 2 cases keep the K-contiguous B the split path requires; the split writes >= 4 partial
        # [M, N] tiles to the head of the registered workspace: proof that it was taken)
        def launch(a, b, Cb, Rb, Xb, o, bias, cscale, aux_layout_nn):
            n = 4 * a.shape[1] * b.shape[1]
            ws[:n].fill_(float("nan"))
            _gemm_launcher(ops, BF)(a, b, Cb, Rb, Xb, o, bias, cscale, False)
            assert not torch.isnan(ws[:n]).any(), "the split-K path not taken"
        _run_all(SHAPES[shape], BF, BF, launch, K=1024)
    finally:
        lib().s2h_gemm_tiny_splitk(prev)


def _mx8_launcher(ops):
    def launch(a, b, Cb, Rb, Xb, o, bias, cscale, aux_layout_nn):
        assert a.shape[0] == 1 and cscale is None and o.get("bias", 0) != 2
        M, N = a.shape[1], b.shape[1]
        qa, qb = ops.mx8_quant(a[0].to(DEV).to(BF)), ops.mx8_quant(b[0].to(DEV).to(BF))
        torch.cuda.synchronize()
        for t, src, rows in ((qa, a[0], M), (qb, b[0], N)):  # the oracle-dequantised operands are the ground truth
            deq = mx.dequantize(t.q.cpu().numpy(), mx.words_to_e8(t.s.cpu().numpy(), rows))
            assert np.array_equal(deq[:, :src.shape[1]], src.double().numpy()) and not deq[:, src.shape[1]:].any()
        ops.gemm_mx8(qa, qb, Cb.view[0], bias=bias, residual=None if Rb is None else Rb.view[0],
                     aux=None if Xb is None else Xb.view[0], aux_mode=o.get("aux", 0), act=o.get("act", NONE),
                     drop_p=o.get("p", 0.0), seed=SEED, drop_idx0=o.get("idx0", 0), alpha=o.get("alpha", 1.0),
                     beta=o.get("beta", 0.0))
    return launch


@pytest.mark.parametrize("c_dtype", [BF, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("shape", ["n72-8col+ragged", "n102-ldc104"])
@pytest.mark.parametrize("cfg", [0, 1, 2, 3])
def test_mx8_epilogue(ops, cfg, shape, c_dtype):
    """s2h_gemm_mx8 shares gemm_epi.h: per-column bias only, no column scale (those option cases run
    with the bias per column and without the scale)"""
    from sam2_video.kernels._lib import lib
    prev = lib().s2h_mx8_config(cfg)
    failures = []
    try:
        for name, o in OPTIONS.items():
            o = dict(o, bias=min(o.get("bias", 0), 1), cscale=False)
            try:
                _run_option(name, o, SHAPES[shape], "mx8", c_dtype, _mx8_launcher(ops), has_cscale=False)
            except AssertionError as e:
                failures.append(str(e))
    finally:
        lib().s2h_mx8_config(prev)
    assert not failures, f"{len(failures)} option case(s) failed:\n" + "\n".join(failures)


def test_wgrad_deterministic_alpha_beta_strided(ops):
    """the deterministic weight-gradient kernel with alpha = 0.75, beta = 1 and a padded dw:
    dw[N, K] = 0.75 dy^T x + dw over 4096 rows of {-1, 0, 1} -- every partial sum and the result are
    exact in fp32, so the output equals the fp64 product"""
    rows, N, K, ld = 4096, 64, 72, 80
    g = _gen("wgrad")
    dy = torch.randint(-1, 2, (rows, N), generator=g).float()
    x = torch.randint(-1, 2, (rows, K), generator=g).float()
    old = torch.randint(-8, 9, (1, N, K), generator=g).float() * 0.25
    dw = Strided(old.to(DEV), ld, 0, 0)
    dyd, xd = dy.to(DEV).to(BF), x.to(DEV).to(BF)
    ops.gemm(dyd, xd, dw.view, M=N, N=K, K=rows, lda_m=1, lda_k=N, ldb_k=K, ldb_n=1, ldc=ld, alpha=0.75, beta=1.0)
    torch.cuda.synchronize()
    ref = 0.75 * (dy.double().t() @ x.double()) + old[0].double()
    assert torch.equal(dw.view[0].double().cpu(), ref)
    assert dw.padding_intact()
