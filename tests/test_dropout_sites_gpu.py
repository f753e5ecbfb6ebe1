"""Every dropout site of libsam2hip against the host model of the counter hash
(oracle/dropout_oracle.py), bit for bit: each case makes the kept values non-zero, reads the mask off the
output's zeros and compares it with keep(fold_seed(seed, rng offset), documented element index, p).
No tolerances.  Each site runs with p in {0.1, 0.5}, an even, an odd and a > 2^33 first index, and the
bound RNG offset at 0 and at a 64-bit value."""
import numpy as np
import pytest
import torch

from oracle import dropout_oracle as dr

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
SEED = 2**40 + 77  # both words of the seed in use
# first element indices: even with the high word set (the pair path), odd (the per-element path), odd
# past 2^33, small even
IDX0 = (2**34 + 6, 7, 2**33 + 5, 10)
OFFSETS = (0, 2**41 + 12345)
PS = (0.1, 0.5)


@pytest.fixture(scope="module")
def ops():
    from sam2_video.kernels import ops as o
    return o


@pytest.fixture(params=OFFSETS, ids=lambda o: f"off{o}")
def off(request, ops):
    t = ops.rng_offset(DEV)
    try:
        t.fill_(request.param)
        yield request.param
    finally:
        t.zero_()
        torch.cuda.synchronize()


def _want(off, idx0, shape, p, seed=SEED):
    """the oracle's keep flags of a dense block of element indices idx0 .. idx0 + prod(shape) - 1"""
    n = int(np.prod(shape))
    idx = np.uint64(idx0) + np.arange(n, dtype=np.uint64)
    return torch.from_numpy(dr.keep(dr.fold_seed(seed, off), idx, p).reshape(shape))


def _check(mask, want, what):
    mask = mask.cpu()
    assert mask.shape == want.shape, (what, mask.shape, want.shape)
    assert torch.equal(mask, want), f"{what}: {int((mask != want).sum())} of {want.numel()} keep flags differ"


def _rand12(*shape):
    g = torch.Generator().manual_seed(sum(shape))
    return (1 + torch.rand(*shape, generator=g)).to(DEV)


# ------------------------------------------------------------------ elementwise
@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("n", [4096, 4099])  # 16-B vector form / scalar form
def test_elementwise_dropout(ops, off, p, dtype, n):
    ones = torch.ones(n, device=DEV, dtype=dtype)
    inv = np.float32(1) / (np.float32(1) - np.float32(p))
    scale = torch.tensor(float(inv), dtype=F32).to(dtype)  # 1 / (1 - p) in fp32, rounded to the dtype
    for idx0 in IDX0:
        want = _want(off, idx0, (n,), p)
        outs = {"s2h_dropout": ops.dropout(ones, p, SEED, idx0=idx0),
                "s2h_act_dropout_bwd": ops.act_dropout_bwd(None, ones, None, p, SEED, idx0=idx0),
                "s2h_act_dropout_bwd+relu": ops.act_dropout_bwd(ones, ones, "relu", p, SEED, idx0=idx0)}
        torch.cuda.synchronize()
        for name, out in outs.items():
            _check(out != 0, want, f"{name} idx0={idx0}")
            assert torch.equal(out.cpu(), torch.where(want, scale, torch.zeros((), dtype=dtype))), name


# ------------------------------------------------------------------ GEMM epilogues
def _gemm_masks(ops, dtype, cdtype, batch, M, N, ldc, K, p, idx0):
    a = torch.zeros(batch, M, K, device=DEV, dtype=dtype)
    g = torch.Generator().manual_seed(N + K)
    b = torch.randn(batch, N, K, generator=g).to(DEV).to(dtype)
    bias = _rand12(N)
    buf = torch.full((batch, M, ldc), -7.0, device=DEV, dtype=cdtype)
    ops.gemm(a, b, buf, M=M, N=N, K=K, lda_m=K, lda_k=1, ldb_k=1, ldb_n=K, ldc=ldc, batch=batch, sA=M * K, sB=N * K,
             sC=M * ldc, bias=bias, drop_p=p, seed=SEED, drop_idx0=idx0)
    torch.cuda.synchronize()
    assert (buf[:, :, N:] == -7.0).all(), "padding columns written"
    return buf[:, :, :N] != 0


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("kind,dtype,cdtype,N,ldc", [("bf16-4col", BF, BF, 102, 104), ("bf16-8col", BF, BF, 64, 72),
                                                     ("bf16-f32out", BF, F32, 102, 104), ("f32", F32, F32, 102, 104)])
def test_gemm_dropout(ops, off, p, kind, dtype, cdtype, N, ldc):
    """index = drop_idx0 + (b*M + m)*N + n: N, not ldc, and the batch term"""
    batch, M, K = 3, 70, 40
    for idx0 in IDX0:
        got = _gemm_masks(ops, dtype, cdtype, batch, M, N, ldc, K, p, idx0)
        _check(got, _want(off, idx0, (batch, M, N), p), f"s2h_gemm {kind} idx0={idx0}")


@pytest.mark.parametrize("p", PS)
def test_gemm_tiny_splitk_dropout(ops, off, p):
    from sam2_video.kernels._lib import lib
    ws = ops.wgrad_workspace(DEV)  # the split needs the registered workspace
    M, N, K = 64, 64, 1024
    x = torch.zeros(M, K, device=DEV, dtype=BF)
    w = torch.randn(N, K, generator=torch.Generator().manual_seed(3)).to(DEV).to(BF)
    bias = _rand12(N)
    prev = lib().s2h_gemm_tiny_splitk(1)
    try:
        for idx0 in IDX0:
            ws[:4 * M * N].fill_(float("nan"))
            y = ops.linear(x, w, bias, drop_p=p, seed=SEED, drop_idx0=idx0)
            torch.cuda.synchronize()
            # (the split writes >= 4 partial [M, N] tiles to the head of the workspace)
            assert not torch.isnan(ws[:4 * M * N]).any(), "the split-K path not taken"
            _check(y != 0, _want(off, idx0, (M, N), p), f"tiny split-K idx0={idx0}")
    finally:
        lib().s2h_gemm_tiny_splitk(prev)


@pytest.mark.parametrize("p", PS)
def test_gemm_mx8_dropout(ops, off, p):
    M, N, ldc, K = 70, 102, 104, 128
    a = ops.mx8_quant(torch.zeros(M, K, device=DEV, dtype=BF))
    b = ops.mx8_quant(torch.randn(N, K, generator=torch.Generator().manual_seed(4)).to(DEV).to(BF))
    bias = _rand12(N)
    for idx0 in IDX0:
        buf = torch.full((M, ldc), -7.0, device=DEV, dtype=BF)
        ops.gemm_mx8(a, b, buf[:, :N], bias=bias, drop_p=p, seed=SEED, drop_idx0=idx0)
        torch.cuda.synchronize()
        assert (buf[:, N:] == -7.0).all()
        _check(buf[:, :N] != 0, _want(off, idx0, (M, N), p), f"s2h_gemm_mx8 idx0={idx0}")


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("N", [128, 256])
def test_linear_add_ln_dropout(ops, off, p, N):
    M, K = 70, 64
    x = torch.zeros(M, K, device=DEV, dtype=BF)
    w = torch.randn(N, K, generator=torch.Generator().manual_seed(5)).to(DEV).to(BF)
    bias = _rand12(N)
    gamma, beta = torch.ones(N, device=DEV), torch.zeros(N, device=DEV)
    for idx0 in IDX0:
        _, xsum, _, _ = ops.linear_add_ln(x, w, bias, None, gamma, beta, 1e-5, drop_p=p, seed=SEED, drop_idx0=idx0)
        torch.cuda.synchronize()
        _check(xsum != 0, _want(off, idx0, (M, N), p), f"s2h_linear_add_ln N={N} idx0={idx0}")


@pytest.mark.parametrize("p", PS)
def test_ffn_fwd_dropout(ops, off, p):
    """hid zeros = the (seed1, idx1 + row*H + h) mask (x = 0, b1 > 0: relu(b1) > 0); y zeros = the
    (seed2, idx2 + row*256 + n) mask (w2 = 0, b2 > 0)"""
    R, H = 64, 1024
    x = torch.zeros(R, 256, device=DEV, dtype=BF)
    w1 = torch.randn(H, 256, generator=torch.Generator().manual_seed(6)).to(DEV).to(BF)
    w2 = torch.zeros(256, H, device=DEV, dtype=BF)
    b1, b2 = _rand12(H), _rand12(256)
    seed2 = SEED ^ 0xABCDEF0123
    assert ops.ffn_fwd_ok(x, w1, b1, w2, b2)
    for idx1, idx2 in zip(IDX0, IDX0[1:] + IDX0[:1]):
        hid, y = ops.ffn_fwd(x, w1, b1, w2, b2, p=p, seed1=SEED, idx1=idx1, seed2=seed2, idx2=idx2)
        torch.cuda.synchronize()
        _check(hid != 0, _want(off, idx1, (R, H), p), f"s2h_ffn_fwd hid idx1={idx1}")
        _check(y != 0, _want(off, idx2, (R, 256), p, seed=seed2), f"s2h_ffn_fwd y idx2={idx2}")


# ------------------------------------------------------------------ attention
SCALE = 0.02  # |scale q.k| << 1: probabilities stay near 1 / Lk, nothing underflows


def _qk(B, H, Lq, Lk, D, dtype):
    g = torch.Generator().manual_seed(Lq * 1000 + Lk)
    q = (torch.randn(B, Lq, H, D, generator=g) * 0.5).to(DEV).to(dtype)
    k = (torch.randn(B, Lk, H, D, generator=g) * 0.5).to(DEV).to(dtype)
    return q, k


def _identity_v(B, H, Lk, D, dtype, k0=0):
    """V[k, d] = [k == k0 + d]: O[q, d] is the dropped, normalised probability of key k0 + d"""
    v = torch.zeros(B, Lk, H, D, device=DEV, dtype=dtype)
    n = min(D, Lk - k0)
    i = torch.arange(n, device=DEV)
    v[:, k0 + i, :, i] = 1
    return v, n


def _unpack(words, rows, Lk):
    """keep words (int32 tensor / uint32 array) -> bool [rows, Lk]"""
    w = words.cpu().numpy().view(np.uint32) if torch.is_tensor(words) else words
    kw = 2 * ((Lk + 63) // 64)
    bits = (w.reshape(rows, kw, 1) >> np.arange(32, dtype=np.uint32)) & 1
    return torch.from_numpy(bits.reshape(rows, kw * 32)[:, :Lk].astype(bool))


def _attn_case(ops, off, dtype, B, H, Lq, Lk, D, p, bitmap=False, chunks=(0,)):
    q, k = _qk(B, H, Lq, Lk, D, dtype)
    lse = torch.empty(B, H, Lq, device=DEV)
    for k0 in chunks:
        v, n = _identity_v(B, H, Lk, D, dtype, k0)
        o = torch.empty(B, Lq, H, D, device=DEV, dtype=dtype)
        ops.attn_fwd(q, k, v, o, lse, SCALE)
        torch.cuda.synchronize()
        assert (o[..., :n] != 0).all(), "a probability underflowed without dropout"
        for idx0 in IDX0:
            keep = torch.zeros(ops.keep_words(B, H, Lq, Lk), device=DEV, dtype=torch.int32) if bitmap else None
            ops.attn_fwd(q, k, v, o, lse, SCALE, p_drop=p, seed=SEED, idx0=idx0, keep=keep)
            torch.cuda.synchronize()
            want = _want(off, idx0, (B, H, Lq, Lk), p)  # idx0 + ((b*H + h)*Lq + q)*Lk + k
            _check(o[..., :n].permute(0, 2, 1, 3) != 0, want[..., k0:k0 + n], f"attention O idx0={idx0} k0={k0}")
            if bitmap:
                _check(_unpack(keep, B * H * Lq, Lk), want.reshape(B * H * Lq, Lk), f"keep bitmap idx0={idx0}")
                model = dr.keep_bitmap(B, H, Lq, Lk, dr.fold_seed(SEED, off), idx0, p)
                assert torch.equal(_unpack(model, B * H * Lq, Lk), want.reshape(B * H * Lq, Lk))


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("dtype", [F32, BF])
def test_attention_generic_dropout(ops, off, p, dtype):
    _attn_case(ops, off, dtype, 2, 2, 20, 24, 32, p)


@pytest.mark.parametrize("p", PS)
def test_attention_flash_dropout(ops, off, p):
    _attn_case(ops, off, BF, 2, 2, 128, 64, 64, p)


@pytest.mark.parametrize("p", PS)
def test_attention_flash_d256_dropout_and_keep_bitmap(ops, off, p):
    _attn_case(ops, off, BF, 2, 2, 128, 200, 256, p, bitmap=True)


@pytest.mark.parametrize("p", PS)
def test_attention_flash_key_split_dropout(ops, off, p):
    """Lk = 512 over several key splits; V is the identity on one 256-key chunk per launch"""
    from sam2_video.kernels._lib import lib
    B, H, Lq, Lk, D = 1, 2, 128, 512, 256
    prev = lib().s2h_attn_config(1 | (256 << 8))
    try:
        assert lib().s2h_attn_fwd_ws_bytes(ops.BF16, B, H, Lq, Lk, D) > 0, "the key split is not taken"
        _attn_case(ops, off, BF, B, H, Lq, Lk, D, p, bitmap=True, chunks=(0, 256))
    finally:
        lib().s2h_attn_config(prev)


@pytest.mark.parametrize("p", PS)
def test_attention_vfold_dropout(ops, off, p):
    B, Lq, Lk = 1, 128, 64
    q, k = _qk(B, 1, Lq, Lk, 256, BF)
    mem = torch.zeros(B, Lk, 1, 64, device=DEV, dtype=BF)
    i = torch.arange(64, device=DEV)
    mem[:, i, 0, i] = 1
    lse = torch.empty(B, 1, Lq, device=DEV)
    u = torch.empty(B, Lq, 1, 72, device=DEV, dtype=BF)
    ops.attn_fwd_vfold(q, k, mem, u, lse, SCALE)
    torch.cuda.synchronize()
    assert (u[..., :64] != 0).all()
    for idx0 in IDX0:
        keep = torch.zeros(ops.keep_words(B, 1, Lq, Lk), device=DEV, dtype=torch.int32)
        ops.attn_fwd_vfold(q, k, mem, u, lse, SCALE, p_drop=p, seed=SEED, idx0=idx0, keep=keep)
        torch.cuda.synchronize()
        want = _want(off, idx0, (B, Lq, Lk), p)  # H = 1
        _check(u[:, :, 0, :64] != 0, want, f"V-fold u idx0={idx0}")
        _check(_unpack(keep, B * Lq, Lk), want.reshape(B * Lq, Lk), f"V-fold keep bitmap idx0={idx0}")
