"""Host model of the dropout counter hash (oracle/dropout_oracle.py) against the contract of
csrc/common.h -- pair structure, seed folding, 64-bit element indices, threshold quantisation, keep rate
and the attention keep-bitmap layout -- and the ops.gemm guard against residual / aux tensors of the
wrong element type.  No GPU."""
import ast
import itertools
import os

import numpy as np
import pytest
import torch

from oracle import dropout_oracle as dr


def _mix32(x):  # scalar python-int restatement of s2h_mix32, independent of the numpy one
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def _hash_pair(seed, pair):
    key = _mix32((seed & 0xFFFFFFFF) ^ 0x5BD1E995) ^ (seed >> 32)
    return _mix32((((pair & 0xFFFFFFFF) + (pair >> 32) * 0x9E3779B9) & 0xFFFFFFFF) ^ key)


def test_oracle_imports_only_numpy():
    src = open(os.path.join(os.path.dirname(dr.__file__), "dropout_oracle.py")).read()
    mods = set()
    for node in ast.walk(ast.parse(src)):
        if isinstance(node, ast.Import):
            mods.update(a.name.split(".")[0] for a in node.names)
        elif isinstance(node, ast.ImportFrom):
            mods.add((node.module or "").split(".")[0])
    assert mods <= {"numpy", "__future__"}, mods


@pytest.mark.parametrize("seed", [0, 77, 1234, 2**40 + 5, 2**64 - 1])
def test_hash_matches_scalar_restatement(seed):
    pairs = [0, 1, 2, 12345, 2**31, 2**32 - 1, 2**32, 2**32 + 1, 2**33 + 2, 2**62 + 12345, 2**63 - 1]
    got = dr.hash_pair(seed, np.array(pairs, dtype=np.uint64))
    assert [int(v) for v in got] == [_hash_pair(seed, p) for p in pairs]
    assert int(dr.mix32(0)) == 0 and int(dr.mix32(1)) == _mix32(1)


@pytest.mark.parametrize("seed", [0, 77, 2**40 + 5])
@pytest.mark.parametrize("p", [0.1, 0.3, 0.5])
def test_pair_structure(seed, p):
    """elements 2i and 2i + 1 take the low / high 16 bits of ONE hash of the pair index i"""
    i = np.concatenate([np.arange(4096, dtype=np.uint64), np.uint64(2**33) + np.arange(4096, dtype=np.uint64)])
    h = dr.hash_pair(seed, i)
    t = np.uint64(dr.threshold16(p))
    assert np.array_equal(dr.keep(seed, 2 * i, p), (h & np.uint64(0xFFFF)) >= t)
    assert np.array_equal(dr.keep(seed, 2 * i + np.uint64(1), p), (h >> np.uint64(16)) >= t)
    # an odd-based run of indices reads the same hashes as the even-based one
    idx = np.arange(1, 8191, dtype=np.uint64)
    both = dr.keep(seed, np.arange(8192, dtype=np.uint64), p)
    assert np.array_equal(dr.keep(seed, idx, p), both[1:8191])


def test_fold_seed():
    for s in (0, 77, 1234, 2**40 + 5, 2**64 - 1):
        assert dr.fold_seed(s, 0) == s
        for off in (1, 12345, 2**40 + 3, 2**64 - 1):
            f = dr.fold_seed(s, off)
            assert f == s ^ ((off * 0x9E3779B97F4A7C15 + 0x632BE59BD9B4E019) % 2**64)
            assert 0 <= f < 2**64 and f != s
    assert dr.fold_seed(5, 1) != dr.fold_seed(5, 2)


def test_threshold_quantisation():
    assert dr.threshold16(0.5) == 1 << 15 and dr.effective_p(0.5) == 0.5
    # float32(0.1) = 0.100000001490116..., times 65536 = 6553.6000977 -> 6553
    assert dr.threshold16(0.1) == 6553 and dr.effective_p(0.1) == 6553 / 65536
    assert dr.threshold16(0.3) == int(float(np.float32(0.3)) * 65536) == 19660
    assert dr.threshold16(0.0) == 0 and dr.keep(3, np.arange(1000, dtype=np.uint64), 0.0).all()
    assert dr.threshold16(1e-6) == 0  # below 1/65536: nothing is dropped
    with pytest.raises(ValueError):
        dr.threshold16(1.0)


@pytest.mark.parametrize("seed", [0, 77, 2**40 + 5])
def test_high_word_of_the_index_is_mixed_in(seed):
    """indices at and above 2^33 (pair indices >= 2^32) do not alias the low ones"""
    n = 1 << 14
    lo = np.arange(n, dtype=np.uint64)
    base = dr.keep(seed, lo, 0.5)
    for hi in (2**33, 2**34, 2**33 + 2**34, 2**63):
        m = dr.keep(seed, lo + np.uint64(hi), 0.5)
        diff = np.count_nonzero(m != base)
        assert abs(diff - n / 2) < 6 * (n / 4) ** 0.5, (hi, diff)  # independent fair bits: n/2 +- 6 sigma
    # and the low word still matters above 2^33
    assert not np.array_equal(dr.keep(seed, lo + np.uint64(2**33), 0.5), dr.keep(seed, lo + np.uint64(2**33 + n), 0.5))


@pytest.mark.parametrize("p,seed,idx0", list(itertools.product([0.1, 0.3, 0.5], [0, 77, 1234, 2**40 + 5],
                                                               [0, 1, 2**33 + 5])))
def test_keep_rate(p, seed, idx0):
    n = 1 << 20
    kept = int(np.count_nonzero(dr.keep(seed, np.uint64(idx0) + np.arange(n, dtype=np.uint64), p)))
    q = dr.effective_p(p)
    sigma = (n * q * (1 - q)) ** 0.5
    dev = abs(kept - n * (1 - q)) / sigma
    print(f"p={p} seed={seed} idx0={idx0}: kept {kept} of {n}, {dev:.2f} sigma")
    assert dev <= 4.0, dev


@pytest.mark.parametrize("B,H,Lq,Lk,idx0", [(2, 2, 5, 24, 0), (1, 1, 3, 200, 7), (1, 2, 4, 64, 2**33 + 5)])
def test_keep_bitmap_layout(B, H, Lq, Lk, idx0):
    seed, p = 1234, 0.3
    w = dr.keep_bitmap(B, H, Lq, Lk, seed, idx0, p)
    kw = 2 * ((Lk + 63) // 64)
    assert w.dtype == np.uint32 and w.shape == (B * H * Lq, kw) and w.size == dr.keep_words(B, H, Lq, Lk)
    flat = w.reshape(-1)
    for b, h, q, k in [(0, 0, 0, 0), (B - 1, H - 1, Lq - 1, Lk - 1), (0, H - 1, 1, min(31, Lk - 2)),
                       (B - 1, 0, 2, Lk // 2), (0, 0, Lq - 1, min(32, Lk - 1))]:
        bit = (int(flat[((b * H + h) * Lq + q) * kw + k // 32]) >> (k & 31)) & 1
        want = bool(dr.keep(seed, np.array([idx0 + ((b * H + h) * Lq + q) * Lk + k], dtype=np.uint64), p)[0])
        assert bool(bit) == want, (b, h, q, k)
    pad = kw * 32 - Lk  # the model leaves the bits of keys >= Lk clear
    if pad:
        bits = (w[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1
        assert not bits.reshape(B * H * Lq, kw * 32)[:, Lk:].any()


# ------------------------------------------------------------------ ops.gemm operand-type guard
def _gemm_args(M=4, N=8, K=8, ab=torch.bfloat16, c=torch.bfloat16):
    a, b = torch.zeros(M, K, dtype=ab), torch.zeros(N, K, dtype=ab)
    out = torch.zeros(M, N, dtype=c)
    return a, b, out, dict(M=M, N=N, K=K, lda_m=K, lda_k=1, ldb_k=1, ldb_n=K, ldc=N)


@pytest.mark.parametrize("ab,c,bad", [(torch.bfloat16, torch.float32, torch.float32),
                                      (torch.bfloat16, torch.bfloat16, torch.float32),
                                      (torch.float32, torch.float32, torch.bfloat16)])
def test_gemm_rejects_residual_and_aux_of_the_wrong_dtype(ab, c, bad):
    """R and X are read as the A / B element type whatever the output type: an fp32 residual handed
    to a bf16 GEMM with an fp32 output would be misread, so ops.gemm refuses it before any launch
    (the check precedes the device check: it raises on host tensors too)"""
    from sam2_video.kernels import ops
    a, b, out, kw = _gemm_args(ab=ab, c=c)
    wrong = torch.zeros(4, 8, dtype=bad)
    with pytest.raises(TypeError, match="residual"):
        ops.gemm(a, b, out, residual=wrong, ldr=8, **kw)
    for mode in (1, 2):
        with pytest.raises(TypeError, match="aux"):
            ops.gemm(a, b, out, aux=wrong, ldx=8, aux_mode=mode, act=1, **kw)
    with pytest.raises(TypeError, match="residual"):
        ops.linear(a, b, residual=wrong, out_dtype=c)
    with pytest.raises(TypeError, match="cscale"):
        ops.gemm(a, b, out, cscale=torch.zeros(8, dtype=torch.bfloat16), **kw)


def test_gemm_mx8_rejects_residual_and_aux_of_the_wrong_dtype():
    from sam2_video.kernels import ops
    M, N, K = 4, 8, 128
    a = ops.MX8(torch.zeros(M, K, dtype=torch.uint8), torch.zeros(1, M, dtype=torch.int32), K)
    b = ops.MX8(torch.zeros(N, K, dtype=torch.uint8), torch.zeros(1, N, dtype=torch.int32), K)
    out = torch.zeros(M, N, dtype=torch.float32)
    wrong = torch.zeros(M, N, dtype=torch.float32)
    with pytest.raises(TypeError, match="residual"):
        ops.gemm_mx8(a, b, out, residual=wrong)
    with pytest.raises(TypeError, match="aux"):
        ops.gemm_mx8(a, b, out, aux=wrong, aux_mode=1)
