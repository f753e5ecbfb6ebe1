"""CPU checks of the exact-integer GEMM cases (gemm_exact_cases.py): the input conditions of every
operand key test_gemm_exact_gpu.py uses, the tag decoder against csrc/gemm16.h's formula, the models
of the two split plans, the table of forced tilings, and the comparison helper against planted defects."""
import re

import pytest
import torch

import gemm_exact_cases as gx

BF, F32 = gx.BF, gx.F32

SPLIT_K = (1032, 2056, 8200)
# (class, batch, M, N, K) of every GPU case
KEYS = sorted(set(
    [("tern" if r[5] == BF else "wide", r[0], r[1], r[2], r[3]) for r in gx.RULES.values()] +
    [("tern", 1) + shp for ins, out in gx.CLASSES.values() for shp in (ins, out, (128,) + ins[1:])] +
    [(c, 1, M, N, K) for c in ("tern", "wide") for M, N in (gx.SHAPE_RAGGED, gx.SHAPE_PARTIAL) for K in gx.K_LIST] +
    [(c, 3, 264, 136, K) for c in ("tern", "wide") for K in (72, 520, 1096)] +
    [(c, 1, M, N, K) for c in ("tern", "wide") for M, N in (gx.SHAPE_RAGGED, gx.SHAPE_PARTIAL) for K in (0, 1, 5, 67, 515)] +
    [("wide", b, M, N, K) for b, M, N in ((3, 264, 136), (1, 8, 136), (1, 264, 24), (1, 264, 136)) for K in SPLIT_K] +
    [("wide", 1, 264, 136, K) for K in gx.WG_K + (gx.wg_k_last8()[0], gx.wg_k_fewer()[0])] +
    [("wide", 1, 336, 112, 20000), ("wide", 1, 130, 77, 4099)] +
    [("tern", 1, M, N, K) for M in (8, 104) for N in (72, 101) for K in (1024, 2048)] +
    [(c, 3, 100, 37, 1) for c in ("tern", "wide")] + [("tern", 1, 104, 136, K) for K in gx.K_LIST] +
    [("wide", 1, M, N, K) for M, N in (gx.SHAPE_RAGGED, gx.SHAPE_PARTIAL) for K in (1, 3, 4, 5, 72, 130, 1037)] +
    [("mx", 1, M, N, K) for M, N in (gx.SHAPE_RAGGED, gx.SHAPE_PARTIAL) for K in (32, 128, 136, 264, 520, 1096)]))


@pytest.mark.parametrize("cls", ["tern", "wide", "mx"])
def test_operand_conditions(cls):
    """the builder's assertions hold for every key, and restated here: integer operands in the class's
    range, |acc| <= 256 (tern, mx: the result is a bf16 value), 254 K < 2^24 and the non-representable
    shares (wide)"""
    lim = {"tern": (1, 1), "wide": (2, 127), "mx": (2, 2)}[cls]
    for key in [k for k in KEYS if k[0] == cls]:
        a, b, acc = gx.operands(*key)
        K = key[4]
        assert a.shape == (key[1], key[2], K) and b.shape == (key[1], key[3], K)
        if K == 0:
            assert not acc.any()
            continue
        for t, m in ((a, lim[0]), (b, lim[1])):
            assert torch.equal(t, t.round()) and t.abs().max() <= m
        if acc.numel() * K <= 10 ** 8:  # (the large shape-rule cases: the builder's own product only)
            assert torch.equal(acc, torch.einsum("bmk,bnk->bmn", a.double(), b.double()))
        if cls == "wide":
            assert lim[0] * lim[1] * K < 2 ** 24
            if K >= 64:
                assert (~gx.bf16_representable(acc)).double().mean() >= 0.5, key
                head = torch.einsum("bmk,bnk->bmn", a[:, :, :64].double(), b[:, :, :64].double())
                assert (~gx.bf16_representable(head)).double().mean() >= 0.5, key
        else:
            assert acc.abs().max() <= 256 and bool(gx.bf16_representable(acc).all()), key
            assert torch.equal(gx.expected(acc, BF).double(), acc)
    if cls == "mx":  # both signs and magnitudes of {-2..2} occur
        a = gx.operands("mx", 1, 264, 136, 520)[0]
        assert sorted(a.unique().tolist()) == [-2, -1, 0, 1, 2]


def test_operands_cached_and_seeded_by_key():
    a0 = gx.operands("tern", 1, 70, 24, 72)
    assert gx.operands("tern", 1, 70, 24, 72) is a0
    assert not torch.equal(a0[0][:, :, :64], gx.operands("tern", 1, 70, 24, 64)[0])


def test_expected_alpha_beta_exact():
    _, _, acc = gx.operands("wide", 1, 264, 136, 8200)
    cold = gx.old_output(1, 264, 136)
    assert torch.equal(cold * 4, (cold * 4).round()) and cold.abs().max() <= 2
    for alpha in (0.5, 0.75, 1.0):
        for beta in (0.0, 1.0):
            want = gx.expected(acc, F32, alpha, beta, cold)
            assert want.dtype == F32 and torch.equal(want.double(), alpha * acc + beta * cold.double())
    with pytest.raises(AssertionError):
        gx.expected(acc, F32, 1.0 / 3.0, 0.0, cold)


def _gemm16_h_tag(BM, BN, WGM, WGN, NS, BK, akc, bkc, regs, mx8, areg=False):
    """csrc/gemm16.h gemm_tag, written out"""
    return (BM | (BN << 10) | (WGM << 20) | (WGN << 24) | (NS << 28) | ((BK // 32) << 32) | (int(akc) << 36) |
            (int(bkc) << 37) | (int(regs) << 38) | (int(mx8) << 39) | (int(areg) << 40))


def test_decode_tag():
    for BM, BN, WGM, WGN, NS, BK in [v[1:] for v in gx.FORCED.values()] + [(256, 256, 2, 4, 2, 64), (64, 64, 2, 2, 2, 128)]:
        for akc in (False, True):
            for bkc in (False, True):
                for regs, mx8, areg, wg in ((0, 0, 0, 0), (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1)):
                    tag = _gemm16_h_tag(BM, BN, WGM, WGN, NS, BK, akc, bkc, regs, mx8, areg) | (wg << 41)
                    assert tag == gx.make_tag(BM, BN, WGM, WGN, NS, BK, akc, bkc, bool(regs), bool(mx8), bool(areg), bool(wg))
                    assert gx.decode_tag(tag) == dict(BM=BM, BN=BN, WGM=WGM, WGN=WGN, NS=NS, BK=BK, akc=akc, bkc=bkc,
                                                      regs=bool(regs), mx8=bool(mx8), areg=bool(areg), wgdet=bool(wg))
    assert gx.decode_tag(0)["BM"] == 0


def test_forced_table():
    """every forced configuration number has exactly one expected tiling, whose name states it"""
    assert sorted(gx.FORCED) == list(range(1, 31)) and set(gx.FORCED_NUMBERS) == set(gx.FORCED) | {-1}
    assert len({v[0] for v in gx.FORCED.values()}) == 30
    for n, (name, BM, BN, WGM, WGN, NS, BK) in gx.FORCED.items():
        assert name.startswith("CFG_")
        m = re.match(r"CFG_(\d+)(?:x(\d+))?", name)
        assert (BM, BN) == (int(m.group(1)), int(m.group(2) or m.group(1))), name
        areg = name.endswith("AREG")
        assert BK == (32 if "K32" in name else 64), name
        ns = re.search(r"NS(\d)", name)
        assert NS == (int(ns.group(1)) if ns else 1 if areg else 2), name
        if "W41" in name or areg:
            assert (WGM, WGN) == (4, 1), name
        assert WGM * WGN in (4, 8) and BM % (16 * WGM) == 0 and BN % (16 * WGN) == 0
        assert 2 * BK * (BM + BN) * (1 if areg else NS) <= 160 * 1024, name  # the ring fits the LDS
    # the dispatch's fallbacks
    assert gx.forced_tag(1, 264, 136, 72, "nt") == (gx.cfg_tag(1, "nt"), True)
    assert gx.forced_tag(1, 70, 24, 72, "tn") == (gx.regs_tag(70, 24, 72, "tn"), False)  # M = 70 is contiguous
    assert gx.forced_tag(1, 70, 24, 72, "nn")[1]
    assert gx.forced_tag(29, 264, 136, 264, "nt") == (gx.cfg_tag(2, "nt"), False)
    assert gx.forced_tag(30, 264, 136, 72, "tn") == (gx.cfg_tag(2, "tn"), False)
    assert gx.decode_tag(gx.forced_tag(29, 264, 136, 72, "nn")[0])["areg"]
    assert gx.decode_tag(gx.forced_tag(-1, 264, 136, 1096, "nt")[0])["BM"] == 128
    for cfg in gx.FORCED_NUMBERS:  # at least one case of test_forced_tiling runs on the configuration's own tiling
        assert any(gx.forced_tag(cfg, M, N, K, lay)[1] for M, N in (gx.SHAPE_RAGGED, gx.SHAPE_PARTIAL)
                   for lay in gx.LAYOUTS for K in gx.K_LIST), cfg


def test_k_list_reasons():
    """the stage / ring arithmetic the K list is chosen for"""
    stages = lambda K, BK: (K // BK, K % BK)  # noqa: E731
    assert stages(8, 64) == (0, 8) and stages(64, 64) == (1, 0) and stages(72, 64) == (1, 8)
    assert stages(120, 64) == (1, 56) and stages(120, 32) == (3, 24)
    assert stages(264, 64) == (4, 8) and stages(264, 32) == (8, 8)      # 4 > 3-deep ring; the 8-deep K32 ring once
    assert stages(520, 64) == (8, 8) and stages(520, 32) == (16, 8)     # 2 x 4-deep, 2 x 8-deep
    assert stages(1096, 64) == (17, 8) and 1096 >= 1024
    assert all(K % 8 == 0 for K in gx.K_LIST)  # the LDS-DMA path's requirement; other K run register-staged


def test_plan_splits_model():
    """gemm_bf16.h plan_splits: s = min(ceil(target / tiles), K / 512, 256); kchunk = ceil(K / s) rounded up to
    64; splits = ceil(K / kchunk)"""
    assert gx.plan_splits(264, 136, 1096, 1, 64, 64, 768) == (2, 576, 264 * 136)
    assert gx.plan_splits(264, 136, 1000, 1, 64, 64, 768)[0] == 1      # K < 1024
    assert gx.plan_splits(4096, 4096, 2048, 1, 64, 64, 768)[0] == 1   # >= 512 tiles
    for batch, M, N, BM, BN in ((3, 264, 136, 64, 64), (1, 8, 136, 64, 64), (1, 264, 24, 64, 64), (1, 264, 136, 128, 64)):
        for K, want, got in ((1032, 2, 2), (2056, 4, 4), (8200, 16, 15)):
            t = gx.split_target_for(M, N, K, batch, BM, BN, want)
            splits, kchunk, per = gx.plan_splits(M, N, K, batch, BM, BN, t)
            assert (splits, kchunk, per) == (got, 576, batch * M * N)
            assert kchunk % 64 == 0 and (splits - 1) * kchunk < K <= splits * kchunk
            if K == 2056:  # a smaller target plans fewer
                assert gx.plan_splits(M, N, K, batch, BM, BN, t - 1)[0] == 3
    assert gx.plan_splits(8, 136, 2056, 1, 64, 64, 12, rowsum=True)[2] == 8 * 136 + 8


def test_wg_plan_model():
    """gemm_wgrad.hip wg_launch: kchunk = ceil(K / s) rounded up to 64, splits = ceil(K / kchunk)"""
    assert gx.wg_plan(4104, 7) == (7, 640, 264)
    assert gx.wg_plan(16392, 16) == (16, 1088, 72)
    assert gx.wg_plan(520, 1) == (1, 576, 520)
    assert [gx.wg_smax(K) for K in gx.WG_K] == [4, 2, 8, 32]
    K, s = gx.wg_k_last8()
    assert gx.wg_plan(K, s)[0] == s and gx.wg_plan(K, s)[2] == 8 and s <= gx.wg_smax(K) and K % 8 == 0
    K, s = gx.wg_k_fewer()
    assert gx.wg_plan(K, s)[0] < s <= gx.wg_smax(K) and K % 8 == 0
    for K in gx.WG_K:
        for s in gx.WG_SPLITS:
            splits, kchunk, last = gx.wg_plan(K, s)
            assert 0 < last <= kchunk and (splits - 1) * kchunk + last == K and splits <= s
    assert sorted(gx.WG_TILES) == list(range(6))
    assert gx.decode_tag(gx.wg_tag(5)) == dict(BM=64, BN=256, WGM=1, WGN=8, NS=3, BK=64, akc=False, bkc=False,
                                               regs=False, mx8=False, areg=False, wgdet=True)


def test_strided_padding():
    v = torch.arange(24.0).reshape(2, 3, 4)
    s = gx.Strided(v, 12, float("nan"), "cpu", off=1, pad=8, dtype=BF)
    assert torch.equal(s.view.float(), v) and s.padding_intact()
    assert s.flat.numel() == 16 + 1 + 2 * (3 * 12 + 8) + 16 and int(s.valid.sum()) == 24
    assert torch.isnan(s.flat[:17]).all() and torch.isnan(s.flat[-16:]).all()
    s.flat[17 + 4] = 0.0  # one padding element written
    assert not s.padding_intact()
    o = gx.Strided(v, 4, gx.SENT, "cpu")
    assert o.padding_intact()
    o.flat[-1] = 0.0
    assert not o.padding_intact()


def _cpu_gemm(a, b, drop=None, double=None, round_at=None, ld_extra=0):
    """a CPU "kernel" over NaN-padded operands with one planted defect: product (m, n, k) dropped / counted
    twice, the partial over k < round_at kept as bf16, or `ld_extra` padded columns read"""
    K = a.shape[2]
    ap = torch.full((a.shape[0], a.shape[1], K + 8), float("nan"), dtype=torch.float64)
    bp = torch.full((b.shape[0], b.shape[1], K + 8), float("nan"), dtype=torch.float64)
    ap[:, :, :K], bp[:, :, :K] = a, b
    if round_at:
        head = torch.einsum("bmk,bnk->bmn", ap[:, :, :round_at], bp[:, :, :round_at]).float().to(BF).double()
        out = head + torch.einsum("bmk,bnk->bmn", ap[:, :, round_at:K], bp[:, :, round_at:K])
    else:
        out = torch.einsum("bmk,bnk->bmn", ap[:, :, :K], bp[:, :, :K])
    for sign, at in ((-1, drop), (1, double)):
        if at:
            m, n, k = at
            out[0, m, n] += sign * ap[0, m, k] * bp[0, n, k]
    if ld_extra:  # row 5 of A read one padded column too far: reaches every output of that row
        out[0, 5, :] += ap[0, 5, K] * bp[0, :, K - 1]
    return out.float()


def test_mismatch_names_planted_defects():
    a, b, acc = gx.operands("wide", 1, 70, 24, 520)
    want = gx.expected(acc, F32)
    assert gx.mismatch(_cpu_gemm(a, b), want, "clean") is None
    k = next(k for k in range(520) if a[0, 9, k] * b[0, 17, k] != 0)
    prod = float(a[0, 9, k] * b[0, 17, k])
    for what, kw, diff in (("dropped", dict(drop=(9, 17, k)), -prod), ("doubled", dict(double=(9, 17, k)), prod)):
        msg = gx.mismatch(_cpu_gemm(a, b, **kw), want, what)
        assert msg.startswith(f"{what}: 1 of {70 * 24} elements differ; first at (0, 9, 17):"), msg
        assert msg.endswith(f"got - want {diff:.9g}"), msg
    msg = gx.mismatch(_cpu_gemm(a, b, round_at=64), want, "rounded")  # > half of the 64-deep partials change
    assert int(re.search(r"(\d+) of", msg).group(1)) >= 70 * 24 // 2, msg
    first = torch.nonzero(~gx.bf16_representable(torch.einsum("bmk,bnk->bmn", a[:, :, :64].double(), b[:, :, :64].double())))[0]
    assert f"first at {tuple(int(x) for x in first)}" in msg, msg
    msg = gx.mismatch(_cpu_gemm(a, b, ld_extra=1), want, "nan")
    assert msg.startswith("nan: 24 of 1680 elements differ; first at (0, 5, 0): got nan"), msg
    # a bf16 output: one product lost from a tern sum is a whole bf16 step
    a, b, acc = gx.operands("tern", 1, 70, 24, 520)
    got = gx.expected(acc, BF).clone()
    got[0, 3, 4] = (acc[0, 3, 4] - 1).float().to(BF)
    assert "first at (0, 3, 4)" in gx.mismatch(got, gx.expected(acc, BF), "bf16") and "got - want -1" in gx.mismatch(
        got, gx.expected(acc, BF), "bf16")
