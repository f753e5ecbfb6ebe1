"""Shared pieces of the exact-integer GEMM tests (test_gemm_exact_host.py, test_gemm_exact_gpu.py).

With integer operands every partial sum of a GEMM, in any order, is an exact fp32 integer as long as the
sum of the absolute values of its terms stays below 2^24.  The kernel output then equals the float64
product bit for bit on every tiling, ring depth, split count and reduction tree (the atomic split-K form
included), and any defect of a main loop -- a stale ring slot, a K piece counted twice, a partial tile
kept at reduced precision, a tail left unzeroed -- is a failing `torch.equal`.  No tolerance is chosen.

Operand classes (seeded by zlib.crc32(repr(key)), references in float64 on the CPU, cached per key):
  tern  A, B in {-1, 0, 1}; max|acc| <= 256 asserted, so the result is itself a bf16 value and the
        output rounding of a bf16 C hides nothing.  Every case with a bf16 output.
  wide  A in {-2..2}, B in {-127..127}; 254 K < 2^24 asserted; at least half of the reference (and of the
        product over the first 64 k) is asserted NOT representable in bf16, so a partial kept at reduced
        precision cannot pass.  Every case with an fp32 output.  (Reductions shorter than 64 cannot meet
        the share -- K = 1 products are <= 254, all bf16 values -- and have no partial to round: the
        share is asserted from K = 64 on.)
  mx    A, B in {-2..2} (exact in MX-fp8: the block scale is 2^-7, the codes +-128 / +-256), zero
        with probability 1/2 so that max|acc| <= 256 holds up to K = 1096 for a bf16 output.

Every operand and output is a strided view inside a flat buffer filled with a sentinel, with at least
16 elements before and after: NaN for operands (row padding, batch padding, both guards: a read beyond
K, M or N hits NaN inside the allocation and poisons an output), -9.0 for outputs (must survive)."""
import zlib

import torch

BF, F32 = torch.bfloat16, torch.float32
SENT = -9.0  # fills every output element no launch may write (exact in bf16)
GUARD = 16   # sentinel elements before and after every view

# K of the LDS-DMA tilings (stage depth 32 / 64, ring depth 2 / 3 / 4 / 8)
K_LIST = (8,      # one partial stage
          64,     # whole stages, no tail
          72,     # one stage and an 8-wide tail
          120,    # a 56-wide tail; BK 32: three stages and a 24-wide tail
          264,    # 4 * 64 + 8: wraps the 2- and 3-deep rings, fills the 8-deep K32 ring once plus a tail
          520,    # 8 * 64 + 8: wraps the 4-deep ring twice and the 8-deep K32 ring twice
          1096)   # 17 * 64 + 8: odd stage count; K >= 1024 is GEMM class 0 and the split regime
SHAPE_RAGGED = (264, 136)  # ragged against 64, 128 and 256
SHAPE_PARTIAL = (70, 24)   # one partial tile, N < 64
LAYOUTS = ("nt", "nn", "tn", "tt")  # A: n = [M, K] K-contiguous, t = [K, M]; B: t = [N, K] K-contiguous, n = [K, N]


def gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def bf16_representable(x):
    return x.float().to(BF).double() == x.double()


_OPERANDS = {}


def operands(cls, batch, M, N, K):
    """(A [batch, M, K], B [batch, N, K] as fp32 CPU tensors, their exact product [batch, M, N] in fp64)"""
    key = (cls, batch, M, N, K)
    if key in _OPERANDS:
        return _OPERANDS[key]
    g = gen("gemm-exact", *key)
    if K == 0:  # an empty reduction: the product is zero
        _OPERANDS[key] = (torch.zeros(batch, M, 0), torch.zeros(batch, N, 0), torch.zeros(batch, M, N).double())
        return _OPERANDS[key]
    if cls == "tern":
        a = torch.randint(-1, 2, (batch, M, K), generator=g).float()
        b = torch.randint(-1, 2, (batch, N, K), generator=g).float()
    elif cls == "wide":
        a = torch.randint(-2, 3, (batch, M, K), generator=g).float()
        b = torch.randint(-127, 128, (batch, N, K), generator=g).float()
    elif cls == "mx":
        a = (torch.randint(-2, 3, (batch, M, K), generator=g) * torch.randint(0, 2, (batch, M, K), generator=g)).float()
        b = (torch.randint(-2, 3, (batch, N, K), generator=g) * torch.randint(0, 2, (batch, N, K), generator=g)).float()
    else:
        raise ValueError(cls)
    acc = a.double() @ b.double().transpose(1, 2)
    if cls == "wide":
        assert 254 * K < 2 ** 24, key
        if K >= 64:
            assert (~bf16_representable(acc)).double().mean() >= 0.5, ("bf16-representable reference", key)
            head = a[:, :, :64].double() @ b[:, :, :64].double().transpose(1, 2)
            assert (~bf16_representable(head)).double().mean() >= 0.5, ("bf16-representable 64-deep partial", key)
    else:
        assert acc.abs().max() <= 256, (key, float(acc.abs().max()))
    _OPERANDS[key] = (a, b, acc)
    return _OPERANDS[key]


def old_output(batch, M, N, *key):
    """C_old: multiples of 0.25 in [-2, 2] (exact in bf16 and fp32)"""
    return torch.randint(-8, 9, (batch, M, N), generator=gen("c-old", batch, M, N, *key)).float() * 0.25


def expected(acc, c_dtype, alpha=1.0, beta=0.0, cold=None):
    """alpha * acc + beta * C_old, exact in fp32 (asserted), as the output type"""
    want = alpha * acc
    if beta != 0.0:
        want = want + beta * cold.double()
    assert torch.equal(want.float().double(), want), "the expected value is not exact in fp32"
    if alpha != 1.0 or beta != 0.0:
        # alpha in {0.5, 0.75}, C_old a multiple of 0.25: every term and every sum is a multiple of 2^-4
        # below 2^24 * 2^-4 -- no rounding in any order
        assert torch.equal((want * 16).round(), want * 16) and float(acc.abs().max()) * 16 < 2 ** 24
    return want.float().to(c_dtype)


class Strided:
    """a [batch, R, C] view (strides sb, ld, 1), `off` elements past GUARD sentinels, inside a flat
    sentinel-filled buffer with GUARD more after the last batch's padding"""

    def __init__(self, values, ld, fill, device, off=0, pad=0, dtype=None):
        dtype = dtype or values.dtype
        batch, R, C = values.shape
        assert ld >= C
        self.ld, self.sb, self.off = ld, R * ld + pad, GUARD + off
        n = self.off + batch * self.sb + GUARD
        self.fill = fill
        self.flat = torch.full((n,), fill, device=device, dtype=dtype)
        self.view = torch.as_strided(self.flat, (batch, R, C), (self.sb, ld, 1), self.off)
        self.view.copy_(values.to(dtype))
        self.valid = torch.zeros(n, dtype=torch.bool, device=device)
        torch.as_strided(self.valid, (batch, R, C), (self.sb, ld, 1), self.off).fill_(True)

    def padding_intact(self):
        p = self.flat[~self.valid]
        return bool(torch.isnan(p).all()) if self.fill != self.fill else bool((p == self.fill).all())


def mismatch(got, want, what):
    """None when got == want element for element (NaN never equal), else the failure message: the count
    of bad elements, the first index, got / want there and got - want, which for integer operands names
    the lost or doubled product"""
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if torch.equal(got, want):
        return None
    bad = ~(got == want)
    i = tuple(int(x) for x in torch.nonzero(bad)[0])
    g, w = float(got[i]), float(want[i])
    return (f"{what}: {int(bad.sum())} of {bad.numel()} elements differ; first at {i}: got {g:.9g} want {w:.9g} "
            f"got - want {g - w:.9g}")


# ---------------------------------------------------------------- profiler tags (csrc/gemm16.h gemm_tag)
def make_tag(BM, BN, WGM, WGN, NS, BK, akc, bkc, regs=False, mx8=False, areg=False, wgdet=False):
    return (BM | BN << 10 | WGM << 20 | WGN << 24 | NS << 28 | (BK // 32) << 32 | int(akc) << 36 | int(bkc) << 37 |
            int(regs) << 38 | int(mx8) << 39 | int(areg) << 40 | int(wgdet) << 41)


def decode_tag(tag):
    bit = lambda b: bool((tag >> b) & 1)  # noqa: E731
    return dict(BM=tag & 0x3FF, BN=(tag >> 10) & 0x3FF, WGM=(tag >> 20) & 0xF, WGN=(tag >> 24) & 0xF,
                NS=(tag >> 28) & 0xF, BK=32 * ((tag >> 32) & 0xF), akc=bit(36), bkc=bit(37), regs=bit(38), mx8=bit(39),
                areg=bit(40), wgdet=bit(41))


# s2h_gemm_config number -> (name in csrc/gemm_bf16.h GemmCfg, BM, BN, WGM, WGN, NS, BK)
FORCED = {
    1: ("CFG_64", 64, 64, 2, 2, 2, 64), 2: ("CFG_128", 128, 128, 2, 2, 2, 64), 3: ("CFG_128_NS3", 128, 128, 2, 2, 3, 64),
    4: ("CFG_256x128", 256, 128, 4, 2, 2, 64), 5: ("CFG_256", 256, 256, 2, 4, 2, 64),
    6: ("CFG_128x256", 128, 256, 2, 4, 2, 64), 7: ("CFG_128x64", 128, 64, 2, 2, 2, 64),
    8: ("CFG_64x128", 64, 128, 2, 2, 2, 64), 9: ("CFG_64_NS3", 64, 64, 2, 2, 3, 64),
    10: ("CFG_64_K32_NS4", 64, 64, 2, 2, 4, 32), 11: ("CFG_128x64_K32_NS3", 128, 64, 2, 2, 3, 32),
    12: ("CFG_128x64_K32_NS4", 128, 64, 2, 2, 4, 32), 13: ("CFG_128x64_NS3", 128, 64, 2, 2, 3, 64),
    14: ("CFG_256x128_W4_K32_NS3", 256, 128, 2, 2, 3, 32), 15: ("CFG_256x128_W4_K64", 256, 128, 2, 2, 2, 64),
    16: ("CFG_128_K32_NS3", 128, 128, 2, 2, 3, 32), 17: ("CFG_256x64_W4_K32_NS3", 256, 64, 4, 1, 3, 32),
    18: ("CFG_64_NS4", 64, 64, 2, 2, 4, 64), 19: ("CFG_64_K32_NS8", 64, 64, 2, 2, 8, 32),
    20: ("CFG_64_W41", 64, 64, 4, 1, 2, 64), 21: ("CFG_128x64_W41", 128, 64, 4, 1, 2, 64),
    22: ("CFG_128x64_W41_K32_NS3", 128, 64, 4, 1, 3, 32), 23: ("CFG_64_W41_NS4", 64, 64, 4, 1, 4, 64),
    24: ("CFG_128x64_W41_NS3", 128, 64, 4, 1, 3, 64), 25: ("CFG_64x256_W41_NS4", 64, 256, 4, 1, 4, 64),
    26: ("CFG_64x128_W41_NS4", 64, 128, 4, 1, 4, 64), 27: ("CFG_64x256_W41_NS3", 64, 256, 4, 1, 3, 64),
    28: ("CFG_64x256_W41_K32_NS4", 64, 256, 4, 1, 4, 32), 29: ("CFG_64_AREG", 64, 64, 4, 1, 1, 64),
    30: ("CFG_64x128_AREG", 64, 128, 4, 1, 1, 64),
}
FORCED_NUMBERS = tuple(range(1, 31)) + (-1,)


def cfg_tag(cfg, layout):
    """the tag of tiling `cfg` (a FORCED number) on operands of `layout`"""
    _, BM, BN, WGM, WGN, NS, BK = FORCED[cfg]
    areg = cfg in (29, 30)
    return make_tag(BM, BN, WGM, WGN, NS, BK, areg or layout[0] == "n", layout[1] == "t", areg=areg)


def glds_ok(M, N, K, layout, aligned=True):
    """gemm_bf16.h gemm_glds_ok for operands whose bases, row pitches and batch strides are multiples of 8
    elements (`aligned`): the contiguous extent of each operand a multiple of 8, K > 0"""
    aext = K if layout[0] == "n" else M
    bext = K if layout[1] == "t" else N
    return aligned and K > 0 and aext % 8 == 0 and bext % 8 == 0


def regs_tag(M, N, K, layout, batch=1):
    """the register-staged kernel's tile (gemm_cfg1.hip CFG_REGS)"""
    t128 = ((M + 127) // 128) * ((N + 127) // 128) * batch
    big = t128 >= 256 or (M >= 128 and N >= 128 and K >= 1024)
    bm = 128 if big else 64
    return make_tag(bm, bm, 2, 2, 1, 64, layout[0] == "n", layout[1] == "t", regs=True)


def forced_tag(cfg, M, N, K, layout, batch=1, aligned=True):
    """(tag, own): the tag s2h_gemm_bf16 records with s2h_gemm_config(cfg), and whether that is the
    configuration's own tiling.  The fallbacks are the dispatch code's: cfg < 0 or operands the LDS-DMA
    path refuses -> the register-staged kernel; an A-in-registers tiling the shape cannot take (A not
    K-contiguous, K > 256) -> CFG_128 (the last line of s2h_gemm_bf16)"""
    if cfg < 0 or not glds_ok(M, N, K, layout, aligned):
        return regs_tag(M, N, K, layout, batch), cfg < 0
    if cfg in (29, 30) and not (layout[0] == "n" and K <= 256):
        return cfg_tag(2, layout), False
    return cfg_tag(cfg, layout), True


# ---------------------------------------------------------------- shape rules (s2h_gemm_config(0))
# name: (batch, M, N, K, layout, output, expected FORCED number, tiny_config) -- one smallest shape per branch
# of pick_cfg, the w41_of mapping (bf16 outputs) and the A-in-registers rule, derived by reading
# gemm_bf16.hip s2h_gemm_bf16 with its default knobs (w41 1, areg 1, class configurations 0 0 0 0 22 22)
RULES = {
    "M<=128 -> CFG_64_NS4 -> W41": (1, 70, 24, 64, "nt", BF, 23, 0),
    "M<=128 fp32 out -> CFG_64_NS4": (1, 70, 24, 64, "nt", F32, 18, 0),
    "CFG_256 (128 tiles of 256^2 over batch 8)": (8, 1024, 1024, 1024, "nt", BF, 5, 0),
    "CFG_128_K32_NS3 (M 32768, K 256, N 512)": (1, 32768, 512, 256, "nt", BF, 16, 0),
    "CFG_128 (K 1024, 512 tiles of 128^2)": (1, 8192, 1016, 1024, "nt", BF, 2, 0),
    "CFG_128x64_K32_NS3 (K > 256, N <= 256) -> W41": (1, 32768, 256, 320, "nt", BF, 22, 0),
    "CFG_128x64_K32_NS3 (K <= 256, 2048 tiles) -> W41": (1, 32768, 512, 192, "nt", BF, 22, 0),
    "CFG_128x64 (1024 tiles) -> W41": (1, 16384, 512, 320, "nt", BF, 21, 0),
    "CFG_128x64 (split regime, 64 tiles)": (1, 1024, 512, 1024, "nt", F32, 7, 0),
    "CFG_64 -> W41": (1, 264, 136, 64, "nt", BF, 20, 0),
    "CFG_64 fp32 out": (1, 264, 136, 64, "nt", F32, 1, 0),
    "tiny_config CFG_128x64_NS3 -> W41": (1, 104, 136, 64, "nt", BF, 24, 13),
    "A in registers K 8": (1, 264, 136, 8, "nt", BF, 29, 0),
    "A in registers K 72": (1, 264, 136, 72, "nn", BF, 29, 0),
    "A in registers refused (A not K-contiguous) K 72": (1, 264, 136, 72, "tn", BF, 20, 0),
    "A in registers not at M 128": (1, 128, 136, 72, "nt", BF, 23, 0),
    "class 5 overrides A in registers K 136": (1, 264, 136, 136, "nt", BF, 22, 0),
    "class 5 overrides A in registers K 200": (1, 264, 136, 200, "nn", BF, 22, 0),
    "class 5 overrides A in registers K 248": (1, 264, 136, 248, "nt", BF, 22, 0),
    "class 4 (M 65536) overrides A in registers K 8": (1, 65536, 64, 8, "nt", BF, 22, 0),
}

# class: (the smallest shape inside, a shape just outside) as (M, N, K); bf16 outputs, M > 128
CLASSES = {
    0: ((136, 64, 1024), (136, 520, 1024)),
    1: ((8192, 64, 64), (8184, 64, 64)),
    2: ((136, 768, 64), (136, 760, 64)),
    3: ((136, 64, 320), (136, 64, 256)),
    4: ((65536, 64, 8), (65528, 64, 8)),
    5: ((136, 64, 136), (136, 64, 120)),
}


# ---------------------------------------------------------------- split plans
# (the registered workspace is far larger than any plan below: its caps never bind)
def plan_splits(M, N, K, batch, BM, BN, target, rowsum=False):
    """gemm_bf16.h plan_splits for a plain fp32-output GEMM with the workspace registered and not
    binding: (splits, kchunk, per) -- per = floats of one split's partials (tiles + row sums)"""
    tiles = ((M + BM - 1) // BM) * ((N + BN - 1) // BN) * batch
    per = batch * M * N + (batch * M if rowsum else 0)
    if not (tiles < 512 and K >= 1024):
        return 1, K, per
    s = min((target + tiles - 1) // tiles, K // 512, 256)
    if s <= 1:
        return 1, K, per
    kchunk = ((K + s - 1) // s + 63) // 64 * 64
    return (K + kchunk - 1) // kchunk, kchunk, per


def split_target_for(M, N, K, batch, BM, BN, want):
    """the smallest s2h_gemm_split_target at which plan_splits plans `want` splits before rounding"""
    tiles = ((M + BM - 1) // BM) * ((N + BN - 1) // BN) * batch
    assert K // 512 >= want
    return (want - 1) * tiles + 1


def wg_smax(K):
    """the deterministic weight-gradient kernel's own cap on the split count (the cost model's range)"""
    mid = 512 <= K < 1024
    return max(1, min(256, K // (128 if mid else 512)))


def wg_plan(K, s):
    """gemm_wgrad.hip wg_launch with the workspace not binding: (splits, kchunk, rows of the last split)"""
    s = max(s, 1)
    kchunk = ((K + s - 1) // s + 63) // 64 * 64
    splits = (K + kchunk - 1) // kchunk
    return splits, kchunk, K - (splits - 1) * kchunk


WG_TILES = {0: (256, 256, 2, 4, 2), 1: (256, 128, 4, 2, 2), 2: (128, 256, 2, 4, 2), 3: (128, 128, 2, 4, 3),
            4: (256, 64, 4, 2, 3), 5: (64, 256, 1, 8, 3)}
WG_SPLITS = (1, 2, 7, 16)
WG_K = (520, 1032, 4104, 16392)  # 520: the mid rule (512 <= K < 1024, few tiles)


def wg_tag(tile):
    BM, BN, WGM, WGN, NS = WG_TILES[tile]
    return make_tag(BM, BN, WGM, WGN, NS, 64, False, False, wgdet=True)


def wg_k_last8():
    """(K, s): the smallest K >= 1024 (a multiple of 8) and forced split count of WG_SPLITS within the
    kernel's cap whose last split holds exactly 8 valid rows"""
    for K in range(1024, 20000, 8):
        for s in WG_SPLITS:
            splits, _, last = wg_plan(K, s)
            if s > 1 and s <= wg_smax(K) and splits == s and last == 8:
                return K, s
    raise AssertionError("no such K")


def wg_k_fewer():
    """(K, s): the smallest K >= 1024 (a multiple of 8) and forced split count within the kernel's cap for
    which rounding kchunk up to 64 yields fewer splits than forced"""
    for K in range(1024, 20000, 8):
        for s in WG_SPLITS:
            if s <= wg_smax(K) and wg_plan(K, s)[0] < s:
                return K, s
    raise AssertionError("no such K")
