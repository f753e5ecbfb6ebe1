"""TEST INFRASTRUCTURE ONLY -- host model of libsam2hip's counter-based dropout hash, the checker
for every dropout site (GEMM epilogues, s2h_dropout / s2h_act_dropout_bwd, the fused LayerNorm and
FFN forms, attention).  Only tests/ may import this file; the product never does.

The reference draws its dropout masks from torch's Philox stream (nn.Dropout, memory_attention.py:40-48,
transformer.py:304-306), which a fused kernel cannot reproduce element by element: parity with the
reference is statistical only.  What is pinned here is the library's own contract, restated from
csrc/common.h in plain numpy integer arithmetic:

  mix32(x):  x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16   (mod 2^32)
  key(seed) = mix32(lo32(seed) ^ 0x5bd1e995) ^ hi32(seed)
  hash_pair(seed, pair) = mix32((lo32(pair) + hi32(pair) * 0x9E3779B9) ^ key(seed))
  keep(seed, idx, p):  h = hash_pair(seed, idx >> 1); u = idx odd ? h >> 16 : h & 0xffff;
                       kept iff u >= (uint32(float32(p) * 2^32) >> 16)
  fold_seed(seed, off) = off ? seed ^ (off * 0x9E3779B97F4A7C15 + 0x632BE59BD9B4E019) : seed  (mod 2^64)

so the drop probability is quantised to effective_p(p) = floor(float32(p) * 65536) / 65536.
"""
from __future__ import annotations

import numpy as np

_M32 = np.uint64(0xFFFFFFFF)
_M64 = (1 << 64) - 1


def _u64(x):
    """python ints / arrays (any integer dtype, values < 2^64) -> uint64 array"""
    if isinstance(x, np.ndarray):
        return x.astype(np.uint64)
    if isinstance(x, (list, tuple)):
        return np.array([int(v) & _M64 for v in x], dtype=np.uint64)
    return np.array(int(x) & _M64, dtype=np.uint64)


def mix32(x):
    """lowbias32 finaliser on uint64 lanes holding 32-bit values"""
    x = _u64(x) & _M32
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & _M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & _M32
    x = x ^ (x >> np.uint64(16))
    return x


def hash_pair(seed, pair):
    """the 32-bit hash of element pair `pair` (uint64 array) under `seed` (a python int)"""
    seed = int(seed) & _M64
    key = int(mix32((seed & 0xFFFFFFFF) ^ 0x5BD1E995)) ^ (seed >> 32)
    pair = _u64(pair)
    lo, hi = pair & _M32, pair >> np.uint64(32)
    x = (lo + ((hi * np.uint64(0x9E3779B9)) & _M32)) & _M32
    return mix32(x ^ np.uint64(key))


def threshold16(p):
    """the 16-bit drop threshold: uint32(float32(p) * 2^32) >> 16"""
    t = int(float(np.float32(p)) * 4294967296.0)
    if not 0 <= t < (1 << 32):
        raise ValueError(f"drop probability {p} outside [0, 1)")
    return t >> 16


def effective_p(p):
    """the drop probability the kernels realise (quantised to 1/65536)"""
    return threshold16(p) / 65536.0


def keep(seed, idx, p):
    """bool array (idx's shape): element idx is kept under (seed, p)"""
    idx = _u64(idx)
    h = hash_pair(seed, idx >> np.uint64(1))
    u = np.where((idx & np.uint64(1)) != 0, h >> np.uint64(16), h & np.uint64(0xFFFF))
    return u >= np.uint64(threshold16(p))


def fold_seed(seed, offset):
    """the per-launch seed after folding the bound device RNG offset (0 leaves it unchanged)"""
    seed, offset = int(seed) & _M64, int(offset) & _M64
    if offset == 0:
        return seed
    return seed ^ ((offset * 0x9E3779B97F4A7C15 + 0x632BE59BD9B4E019) & _M64)


def keep_words(B, H, Lq, Lk):
    """uint32 words of one attention launch's keep bitmap"""
    return B * H * Lq * 2 * ((Lk + 63) // 64)


def keep_bitmap(B, H, Lq, Lk, seed, idx0, p):
    """the attention keep bitmap, uint32 [B*H*Lq, kw] (kw = 2 * ceil(Lk / 64)): bit (k & 31) of word
    [(b*H + h)*Lq + q]*kw + k/32 = keep(seed, idx0 + ((b*H + h)*Lq + q)*Lk + k, p).  Bits of keys >= Lk are
    clear here; the kernels leave them unspecified (they hash whole 64-key tiles), so compare k < Lk only"""
    kw = 2 * ((Lk + 63) // 64)
    rows = B * H * Lq
    idx = np.uint64(int(idx0) & _M64) + np.arange(rows * Lk, dtype=np.uint64)
    bits = np.zeros((rows, kw * 32), dtype=np.uint64)
    bits[:, :Lk] = keep(seed, idx, p).reshape(rows, Lk)
    w = (bits.reshape(rows, kw, 32) << np.arange(32, dtype=np.uint64)).sum(axis=2)
    return w.astype(np.uint32)
