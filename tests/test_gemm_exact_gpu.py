"""Exact integer pins on the GEMM main loops: every bf16 tiling (csrc/gemm_bf16.h), the shape rules
(gemm_bf16.hip), the register-staged kernel, the generic split-K plan and its atomic form, the
deterministic weight-gradient kernel (gemm_wgrad.hip), the tiny split-K / outer-product paths, the fp32
kernel (gemm.hip) and the MX-fp8 kernel (gemm_mx8.hip).

Integer operands (gemm_exact_cases.py) make every partial sum in any order an exact fp32 integer, so the
output must equal the float64 product bit for bit: the comparison is torch.equal on the valid region.
Every operand lives inside a NaN-filled buffer (row padding of 8 / 24 elements, batch padding, 16-element
guards), so anything read beyond K, M or N reaches an output as NaN; every output lives inside a
-9-filled buffer that must survive.  Every case asserts the path it took from the profiler tag of its
launch (csrc/gemm16.h gemm_tag); split cases also NaN-fill the head of the registered workspace and
assert how much of it the launch overwrote.

The fused launches that share these main loops (s2h_linear_rope, s2h_linear_add_ln,
s2h_linear_dgrad_ln_bwd) have inexact epilogues and are not covered here, nor are the attention GEMMs."""
import contextlib

import numpy as np
import pytest
import torch

import gemm_exact_cases as gx
from oracle import mx8_oracle as mx

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF, F32 = gx.BF, gx.F32
NAN = float("nan")
PROF_CAP = 2048


@pytest.fixture(scope="module")
def ops():
    from sam2_video.kernels import ops as o
    return o


def _lib():
    from sam2_video.kernels import _lib as L
    return L


def lib():
    return _lib().lib()


def _pads(i):
    """operand row padding (A, B) in elements: 8 and 24, swapped from case to case"""
    return (8, 24) if i % 2 == 0 else (24, 8)


_DEV_OPERANDS = {}


def dev_operands(cls, batch, M, N, K, layout, dtype, pads=(8, 24), offA=0, cache=True):
    """the operands of class `cls` as NaN-padded device buffers in `layout` + their ops.gemm strides"""
    key = (cls, batch, M, N, K, layout, dtype, pads, offA)
    if key in _DEV_OPERANDS:
        return _DEV_OPERANDS[key]
    a, b, _ = gx.operands(cls, batch, M, N, K)
    an, bt = layout[0] == "n", layout[1] == "t"
    av = a if an else a.transpose(1, 2)
    bv = b if bt else b.transpose(1, 2)
    bpad = 8 if batch > 1 else 0
    A = gx.Strided(av, av.shape[2] + pads[0], NAN, DEV, off=offA, pad=bpad, dtype=dtype)
    B = gx.Strided(bv, bv.shape[2] + pads[1], NAN, DEV, pad=3 * bpad, dtype=dtype)
    kw = dict(lda_m=A.ld if an else 1, lda_k=1 if an else A.ld, ldb_k=1 if bt else B.ld, ldb_n=B.ld if bt else 1,
              sA=A.sb, sB=B.sb)
    if cache:
        _DEV_OPERANDS[key] = (A, B, kw)
    return A, B, kw


class Session:
    def __init__(self, ops):
        self.ops, self.fails, self.expect, self.skipped = ops, [], [], []

    def note(self, what, want):
        """the next profiler record must carry tag `want` (an int, or a predicate of (tag, meta))"""
        self.expect.append((what, want))

    def check(self, what, C, want):
        wd = want.to(DEV)
        if not torch.equal(C.view, wd):
            self.fails.append(gx.mismatch(C.view, wd, what))
        if not C.padding_intact():
            self.fails.append(f"{what}: padding of the output overwritten")

    def gemm(self, what, cls, M, N, K, layout, c_dtype, tag, *, batch=1, alpha=1.0, beta=0.0, pads=(8, 24), offA=0,
             ldc_pad=8, ab_dtype=BF, cache=True, before=None, after=None):
        _, _, acc = gx.operands(cls, batch, M, N, K)
        A, B, kw = dev_operands(cls, batch, M, N, K, layout, ab_dtype, pads, offA, cache)
        cold = gx.old_output(batch, M, N)
        C = gx.Strided(cold, N + ldc_pad, gx.SENT, DEV, pad=16 if batch > 1 else 0, dtype=c_dtype)
        if before:
            before()
        self.ops.gemm(A.view, B.view, C.view, M=M, N=N, K=K, ldc=C.ld, batch=batch, sC=C.sb, alpha=alpha, beta=beta,
                      **kw)
        self.note(what, tag)
        self.check(what, C, gx.expected(acc, c_dtype, alpha, beta, cold))
        if after:
            after(what)

    def check_tags(self):
        from bench import read_prof
        torch.cuda.synchronize()
        recs = read_prof(_lib(), with_tags=True)
        if len(recs) != len(self.expect):
            self.fails.append(f"{len(self.expect)} launches, {len(recs)} profiler records")
            return
        for (what, want), (_, meta, tag) in zip(self.expect, recs):
            ok = want(tag, meta) if callable(want) else tag == want
            if not ok:
                wanted = "" if callable(want) else f", want {gx.decode_tag(want)}"
                self.fails.append(f"{what}: ran on {gx.decode_tag(tag)} (tag {tag:#x}, record {meta}){wanted}")


@contextlib.contextmanager
def session(ops):
    """profile every GEMM launch inside; on exit compare the tags, restore the profiler's settings (off,
    attention forward selected: the library's defaults) and raise the collected failures"""
    s = Session(ops)
    L = _lib()
    L.call("s2h_prof_enable", PROF_CAP)
    L.call("s2h_prof_select", 4)
    try:
        yield s
        s.check_tags()
    finally:
        L.call("s2h_prof_enable", 0)
        L.call("s2h_prof_select", 1)
    for line in s.skipped:
        print("skipped:", line)
    assert not s.fails, f"{len(s.fails)} case(s) failed:\n" + "\n".join(s.fails[:40])


class Workspace:
    """the registered deterministic-reduction workspace: NaN-fill its head, then assert how much a launch
    overwrote (exact partials are never NaN)"""

    def __init__(self, ops, s):
        self.ws, self.s = ops.wgrad_workspace(DEV), s

    def poison(self, n):
        self.ws[:n + 64].fill_(NAN)

    def written(self, what, n):
        """floats 0 .. n-1 written, the next 64 not"""
        if torch.isnan(self.ws[:n]).any():
            self.s.fails.append(f"{what}: {int(torch.isnan(self.ws[:n]).sum())} of the {n} workspace floats of the plan "
                                f"not written")
        if not torch.isnan(self.ws[n:n + 64]).all():
            self.s.fails.append(f"{what}: workspace written beyond the plan's {n} floats")


# ------------------------------------------------------------------ 1. every forced bf16 tiling
BATCH3_CFGS = (1, 7, 18, 22, 29)


@pytest.mark.parametrize("cfg", gx.FORCED_NUMBERS)
def test_forced_tiling(ops, cfg):
    """s2h_gemm_config(cfg): every layout x K of K_LIST x {264 x 136, 70 x 24} x {bf16 out (tern), fp32 out
    beta 0 / 1 (wide)}; the tag is the configuration's own tiling or the fallback the dispatch names
    (gemm_exact_cases.forced_tag), and at least one case runs on the configuration's own tiling"""
    prev = lib().s2h_gemm_config(cfg)
    own, i = 0, 0
    try:
        with session(ops) as s:
            for M, N in (gx.SHAPE_RAGGED, gx.SHAPE_PARTIAL):
                for layout in gx.LAYOUTS:
                    for K in gx.K_LIST:
                        tag, is_own = gx.forced_tag(cfg, M, N, K, layout)
                        own += is_own
                        i += 1
                        name = f"cfg {cfg} {M}x{N}x{K} {layout}"
                        s.gemm(name + " bf16", "tern", M, N, K, layout, BF, tag, pads=_pads(i))
                        s.gemm(name + " fp32", "wide", M, N, K, layout, F32, tag, pads=_pads(i))
                        s.gemm(name + " fp32 beta 1", "wide", M, N, K, layout, F32, tag, beta=1.0, pads=_pads(i + 1))
            if cfg in BATCH3_CFGS:
                M, N = gx.SHAPE_RAGGED
                for layout in gx.LAYOUTS:
                    for K in (72, 520, 1096):
                        tag, _ = gx.forced_tag(cfg, M, N, K, layout, batch=3)
                        name = f"cfg {cfg} 3x{M}x{N}x{K} {layout}"
                        s.gemm(name + " bf16", "tern", M, N, K, layout, BF, tag, batch=3)
                        s.gemm(name + " fp32 beta 1", "wide", M, N, K, layout, F32, tag, batch=3, beta=1.0)
            assert own > 0, f"configuration {cfg} never ran on its own tiling"
    finally:
        lib().s2h_gemm_config(prev)


# ------------------------------------------------------------------ 2. the shape rules, nothing forced
@pytest.mark.parametrize("rule", list(gx.RULES), ids=list(gx.RULES))
def test_shape_rule(ops, rule):
    batch, M, N, K, layout, c_dtype, cfg, tiny = gx.RULES[rule]
    prev, prev_tiny = lib().s2h_gemm_config(0), lib().s2h_gemm_tiny_config(tiny)
    try:
        with session(ops) as s:
            s.gemm(rule, "tern" if c_dtype == BF else "wide", M, N, K, layout, c_dtype, gx.cfg_tag(cfg, layout),
                   batch=batch, cache=False)
    finally:
        lib().s2h_gemm_config(prev)
        lib().s2h_gemm_tiny_config(prev_tiny)


@pytest.mark.parametrize("cls", list(gx.CLASSES))
def test_gemm_class(ops, cls):
    """gemm_class: with s2h_gemm_class_config(cls, CFG_64_NS3) the smallest shape of the class runs on that
    tiling, a shape just outside (and M = 128) does not"""
    inside, outside = gx.CLASSES[cls]
    tag9 = gx.cfg_tag(9, "nt")
    prev, prev_cls = lib().s2h_gemm_config(0), lib().s2h_gemm_class_config(cls, 9)
    try:
        with session(ops) as s:
            s.gemm(f"class {cls} inside {inside}", "tern", *inside, "nt", BF, tag9, cache=False)
            for shp in (outside, (128,) + inside[1:]):
                s.gemm(f"class {cls} outside {shp}", "tern", *shp, "nt", BF, lambda tag, meta: tag != tag9 and tag != 0,
                       cache=False)
    finally:
        lib().s2h_gemm_config(prev)
        lib().s2h_gemm_class_config(cls, prev_cls)


# ------------------------------------------------------------------ 3. register-staged path
def test_register_staged(ops):
    """the register-staged kernel: K not a multiple of 8 (forced with s2h_gemm_config(-1)), and with
    nothing forced a base offset of 1 element, a row pitch that is no multiple of 8, and K = 0"""
    prev = lib().s2h_gemm_config(-1)
    try:
        with session(ops) as s:
            i = 0
            for M, N in (gx.SHAPE_RAGGED, gx.SHAPE_PARTIAL):
                for layout in gx.LAYOUTS:
                    for K in (1, 5, 67, 515):
                        i += 1
                        tag = gx.regs_tag(M, N, K, layout)
                        name = f"regs {M}x{N}x{K} {layout}"
                        s.gemm(name + " bf16", "tern", M, N, K, layout, BF, tag, pads=_pads(i))
                        s.gemm(name + " fp32", "wide", M, N, K, layout, F32, tag, pads=_pads(i))
                        s.gemm(name + " fp32 beta 1", "wide", M, N, K, layout, F32, tag, beta=1.0, pads=_pads(i + 1))
            lib().s2h_gemm_config(0)
            M, N = gx.SHAPE_RAGGED
            for layout in gx.LAYOUTS:
                for K in (72, 520):
                    tag = gx.regs_tag(M, N, K, layout)
                    for what, kw in (("base + 1", dict(offA=1)), ("pitch + 3", dict(pads=(3, 8))),
                                     ("pitch B + 5", dict(pads=(8, 5)))):
                        name = f"regs {what} {M}x{N}x{K} {layout}"
                        s.gemm(name + " bf16", "tern", M, N, K, layout, BF, tag, **kw)
                        s.gemm(name + " fp32 beta 1", "wide", M, N, K, layout, F32, tag, beta=1.0, **kw)
                # K = 0: beta * C_old for an fp32 output, 0 for bf16
                tag = gx.regs_tag(M, N, 0, layout)
                s.gemm(f"K 0 {layout} bf16", "tern", M, N, 0, layout, BF, tag)
                s.gemm(f"K 0 {layout} fp32", "wide", M, N, 0, layout, F32, tag)
                s.gemm(f"K 0 {layout} fp32 beta 1", "wide", M, N, 0, layout, F32, tag, beta=1.0)
    finally:
        lib().s2h_gemm_config(prev)


# ------------------------------------------------------------------ 4. generic split-K (plan_splits)
# the cases the deterministic weight-gradient kernel refuses: name -> (batch, M, N, layout, forced cfg)
SPLIT_CASES = {
    "batch 3": (3, 264, 136, "tn", 0),
    "M < 16": (1, 8, 136, "tn", 0),
    "N < 64": (1, 264, 24, "tn", 0),
    "forced 128x64": (1, 264, 136, "tn", 7),
    "forced 64x64 K-contiguous": (1, 264, 136, "nt", 1),
}
SPLIT_K = ((1032, 2), (2056, 4), (8200, 16))  # K, the split count planned before kchunk is rounded up to 64


def _split_tile(M, cfg):
    """(FORCED number, BM, BN) of the tiling a split case runs on: pick_cfg's split regime with < 64 tiles of
    128 x 64 is CFG_64, CFG_64_NS4 at M <= 128"""
    n = cfg or (18 if M <= 128 else 1)
    return n, gx.FORCED[n][1], gx.FORCED[n][2]


@pytest.mark.parametrize("atomic", [0, 1], ids=["workspace", "atomic"])
@pytest.mark.parametrize("case", list(SPLIT_CASES), ids=list(SPLIT_CASES))
def test_generic_split_k(ops, case, atomic):
    """plan_splits with s2h_gemm_split_target raised until 2, 4 and 16 splits are planned: beta 0 and 1, alpha
    0.5 / 0.75, a padded ldc; the workspace holds exactly splits * per partial floats -- or, in the atomic
    form (dbg bit 32), stays untouched"""
    batch, M, N, layout, cfg = SPLIT_CASES[case]
    n, BM, BN = _split_tile(M, cfg)
    prev = lib().s2h_gemm_config(cfg | (32 << 8) if atomic else cfg)
    prev_t = lib().s2h_gemm_split_target(0)
    try:
        with session(ops) as s:
            ws = Workspace(ops, s)
            for K, want in SPLIT_K:
                target = gx.split_target_for(M, N, K, batch, BM, BN, want)
                lib().s2h_gemm_split_target(target)
                splits, _, per = gx.plan_splits(M, N, K, batch, BM, BN, target)
                assert splits >= 2
                used = 0 if atomic else splits * per
                for alpha, beta, ldc_pad in ((1.0, 0.0, 0), (0.75, 1.0, 8), (0.5, 0.0, 24)):
                    s.gemm(f"split {case} K {K} x{splits} alpha {alpha} beta {beta}", "wide", M, N, K, layout, F32,
                           gx.cfg_tag(n, layout), batch=batch, alpha=alpha, beta=beta, ldc_pad=ldc_pad,
                           before=lambda: ws.poison(splits * per), after=lambda what: ws.written(what, used))
    finally:
        lib().s2h_gemm_config(prev)
        lib().s2h_gemm_split_target(prev_t)


def _linear_wgrad(s, what, ops, Nl, Kl, rows, accumulate, tag, pads, before=None, after=None):
    """ops.linear_wgrad(dy [rows, Nl], x [rows, Kl], dw, db=) on wide operands: dw and the bias gradient
    (the fused row sums of the GEMM's A) are exact"""
    a, _, acc = gx.operands("wide", 1, Nl, Kl, rows)
    A, B, _ = dev_operands("wide", 1, Nl, Kl, rows, "tn", BF, pads)
    cold = gx.old_output(1, Nl, Kl)
    C = gx.Strided(cold, Kl + 8, gx.SENT, DEV, dtype=F32)
    bold = gx.old_output(1, 1, Nl, "db")
    D = gx.Strided(bold, Nl, gx.SENT, DEV, dtype=F32)
    if before:
        before()
    ops.linear_wgrad(A.view[0], B.view[0], C.view[0], accumulate=accumulate, db=D.view[0, 0])
    s.note(what, tag)
    beta = 1.0 if accumulate else 0.0
    s.check(what + " dw", C, gx.expected(acc, F32, 1.0, beta, cold))
    s.check(what + " db", D, gx.expected(a.double().sum(2)[:, None, :], F32, 1.0, beta, bold))
    if after:
        after(what)


@pytest.mark.parametrize("atomic", [0, 1], ids=["workspace", "atomic"])
def test_generic_split_k_rowsum(ops, atomic):
    """the fused row sum (bias gradient) of a split launch: its partials follow the tiles' in the workspace"""
    prev = lib().s2h_gemm_config((32 << 8) if atomic else 0)
    prev_t = lib().s2h_gemm_split_target(0)
    try:
        with session(ops) as s:
            ws = Workspace(ops, s)
            for Nl, Kl in ((8, 136), (264, 24)):
                n, BM, BN = _split_tile(Nl, 0)
                for K, want in SPLIT_K:
                    target = gx.split_target_for(Nl, Kl, K, 1, BM, BN, want)
                    lib().s2h_gemm_split_target(target)
                    splits, _, per = gx.plan_splits(Nl, Kl, K, 1, BM, BN, target, rowsum=True)
                    used = 0 if atomic else splits * per
                    for acc in (False, True):
                        _linear_wgrad(s, f"split rowsum {Nl}x{Kl} rows {K} x{splits} accumulate {acc}", ops, Nl, Kl, K, acc,
                                      gx.cfg_tag(n, "tn"), _pads(int(acc)), before=lambda: ws.poison(splits * per),
                                      after=lambda what: ws.written(what, used))
    finally:
        lib().s2h_gemm_config(prev)
        lib().s2h_gemm_split_target(prev_t)


# ------------------------------------------------------------------ 5. deterministic weight-gradient kernel
@pytest.mark.parametrize("tile", list(gx.WG_TILES))
def test_wgrad_det_forced(ops, tile):
    """s2h_wgrad_force(tile, splits): splits of WG_SPLITS x K of WG_K, plus one K whose last split holds
    exactly 8 valid rows and one where rounding kchunk up to 64 yields fewer splits than forced; alpha
    0.75 / 1, beta 0 / 1, operand pitches padded by 8 and 24; then with the fused bias gradient through
    ops.linear_wgrad.  A forced split count beyond the kernel's own cap for that K (wg_smax) is skipped."""
    M, N = gx.SHAPE_RAGGED
    BM, BN = gx.WG_TILES[tile][:2]
    ntm, ntn = (M + BM - 1) // BM, (N + BN - 1) // BN
    k8, s8 = gx.wg_k_last8()
    kf, sf = gx.wg_k_fewer()
    combos = [(K, sp) for K in gx.WG_K for sp in gx.WG_SPLITS] + [(k8, s8), (kf, sf)]
    prev = lib().s2h_gemm_config(0)
    try:
        with session(ops) as s:
            ws = Workspace(ops, s)
            for i, (K, sp) in enumerate(combos):
                if sp > gx.wg_smax(K):
                    s.skipped.append(f"tile {tile} K {K}: {sp} forced splits exceed the kernel's cap of {gx.wg_smax(K)}")
                    continue
                lib().s2h_wgrad_force(tile, sp)
                splits = gx.wg_plan(K, sp)[0]
                n = splits * ntm * ntn * BM * BN
                for alpha, beta in ((1.0, 0.0), (0.75, 1.0), (0.75, 0.0), (1.0, 1.0)):
                    s.gemm(f"wgrad tile {tile} K {K} forced {sp} -> {splits} splits alpha {alpha} beta {beta}", "wide", M, N,
                           K, "tn", F32, gx.wg_tag(tile), alpha=alpha, beta=beta, pads=_pads(i),
                           before=lambda: ws.poison(n), after=lambda what: ws.written(what, n))
                nrs = n + splits * ntm * BM
                for acc in (False, True):
                    _linear_wgrad(s, f"wgrad tile {tile} rows {K} forced {sp} -> {splits} splits + db accumulate {acc}", ops,
                                  M, N, K, acc, gx.wg_tag(tile), _pads(i + 1), before=lambda: ws.poison(nrs),
                                  after=lambda what: ws.written(what, nrs))
    finally:
        lib().s2h_wgrad_force(-1, 0)
        lib().s2h_gemm_config(prev)


def test_wgrad_det_unforced(ops):
    """nothing forced: 20000 rows x 336 x 112 takes the deterministic kernel (the cost model's tile), 4099
    rows x 130 x 77 (pitches no multiple of 8) the unaligned fallback: register-staged split-K"""
    prev = lib().s2h_gemm_config(0)
    lib().s2h_wgrad_force(-1, 0)
    try:
        with session(ops) as s:
            for beta in (0.0, 1.0):
                s.gemm(f"wgrad 20000x336x112 beta {beta}", "wide", 336, 112, 20000, "tn", F32,
                       lambda tag, meta: gx.decode_tag(tag)["wgdet"], beta=beta)
                s.gemm(f"wgrad 4099x130x77 beta {beta}", "wide", 130, 77, 4099, "tn", F32,
                       gx.regs_tag(130, 77, 4099, "tn"), beta=beta, pads=(8, 8))
    finally:
        lib().s2h_gemm_config(prev)


# ------------------------------------------------------------------ 6. small paths
def test_tiny_split_k(ops):
    """s2h_gemm_tiny_splitk(1): M <= 128, K >= 1024 as S K-slices of one fp32 launch on CFG_64_NS4 into the
    workspace + the reduce-epilogue launch"""
    prev, prev_s = lib().s2h_gemm_config(0), lib().s2h_gemm_tiny_splitk(1)
    try:
        with session(ops) as s:
            ws = Workspace(ops, s)
            for M in (8, 104):
                for N in (72, 101):
                    for K in (1024, 2048):
                        S = 16  # gemm_bf16.hip gemm_tiny_splitk: K % (64 S) == 0, tiles * S <= 256
                        n = S * M * N
                        s.gemm(f"tiny split-K {M}x{N}x{K}", "tern", M, N, K, "nt", BF, gx.cfg_tag(18, "nt"),
                               ldc_pad=8 if N % 8 == 0 else 0, before=lambda: ws.poison(n),
                               after=lambda what: ws.written(what, n))
    finally:
        lib().s2h_gemm_tiny_splitk(prev_s)
        lib().s2h_gemm_config(prev)


def test_outer_product_and_tiny_config(ops):
    """K = 1: the outer-product kernel (no tiling tag) and the forced 64 x 64 tiling (K = 1 is not a multiple
    of 8: its register-staged fallback) both equal the product, hence each other; s2h_gemm_tiny_config 18 /
    19 at M = 104 over K_LIST"""
    prev = lib().s2h_gemm_config(0)
    try:
        with session(ops) as s:
            for c_dtype, cls in ((BF, "tern"), (F32, "wide")):
                lib().s2h_gemm_config(0)
                s.gemm(f"outer 3x100x37 {c_dtype}", cls, 100, 37, 1, "nt", c_dtype, 0, batch=3, ldc_pad=3)
                lib().s2h_gemm_config(1)
                s.gemm(f"outer on cfg 1 3x100x37 {c_dtype}", cls, 100, 37, 1, "nt", c_dtype,
                       gx.regs_tag(100, 37, 1, "nt", 3), batch=3, ldc_pad=3)
            lib().s2h_gemm_config(0)
            for tiny, want in ((18, 23), (19, 19)):  # w41_of maps CFG_64_NS4 to CFG_64_W41_NS4 for a bf16 output
                lib().s2h_gemm_tiny_config(tiny)
                for layout in gx.LAYOUTS:
                    for K in gx.K_LIST:
                        s.gemm(f"tiny_config {tiny} 104x136x{K} {layout}", "tern", 104, 136, K, layout, BF,
                               gx.cfg_tag(want, layout))
    finally:
        lib().s2h_gemm_tiny_config(0)
        lib().s2h_gemm_config(prev)


# ------------------------------------------------------------------ 7. fp32 kernel (gemm.hip)
F32_K = (1, 3, 4, 5, 72, 130, 1037)


def _f32_rec(tag, meta):
    """the fp32 kernel records no tiling tag; its record's layout word has the bf16 bit (4) clear"""
    return tag == 0 and not (meta[5] & 4)


@pytest.mark.parametrize("small", [1, 0], ids=["32x32", "64x64"])
def test_fp32_kernel(ops, small):
    """fp32 operands (wide), every layout, K of F32_K, beta 0 / 1, on the 32 x 32 (s2h_gemm_f32_small 1:
    fewer than 64 tiles of 64^2) and 64 x 64 tiles"""
    prev = lib().s2h_gemm_f32_small(small)
    try:
        with session(ops) as s:
            i = 0
            for M, N in (gx.SHAPE_RAGGED, gx.SHAPE_PARTIAL):
                for layout in gx.LAYOUTS:
                    for K in F32_K:
                        i += 1
                        for beta in (0.0, 1.0):
                            s.gemm(f"fp32 {M}x{N}x{K} {layout} beta {beta}", "wide", M, N, K, layout, F32, _f32_rec,
                                   beta=beta, pads=_pads(i), ab_dtype=F32, ldc_pad=4)
    finally:
        lib().s2h_gemm_f32_small(prev)


def test_fp32_kernel_128_tiles(ops):
    """batch 128 of 130 x 130: 512 tiles of 128 x 128 (the big-tile rule of launch_gemm), every K on the
    K-contiguous layout, every layout at K = 130"""
    with session(ops) as s:
        for layout, K in [("nt", K) for K in F32_K] + [(lay, 130) for lay in gx.LAYOUTS[1:]]:
            for beta in (0.0, 1.0):
                s.gemm(f"fp32 128x130x130x{K} {layout} beta {beta}", "wide", 130, 130, K, layout, F32, _f32_rec, batch=128,
                       beta=beta, ab_dtype=F32, ldc_pad=2, cache=False)


# ------------------------------------------------------------------ 8. MX-fp8 kernel
MX_K = (32,    # one scale block
        128,   # one whole 128-deep step
        136,   # a step and an 8-wide tail
        264,   # two steps and a tail: the 2-deep ring wraps
        520, 1096)
MX_TILE = {0: (64, 64), 1: (64, 64), 2: (128, 64), 3: (128, 128)}  # 0: the shape rule (small grids: 64 x 64)
E4M3_NAN, E8M0_NAN = 0x7F, -1  # poison of the quantised operands' padding (-1: four 0xFF scale bytes)

_MXQ = {}


def _mx_operand(ops, which, M, N, K):
    """one `mx` operand quantised into poisoned buffers.  The quantiser OWNS and must write every byte of
    q[rows, 0:Kp] (Kp = K rounded up to 128: codes for k < K, ZERO for K <= k < Kp -- the GEMM has no K
    tail and reads them) and the scale words s[0:Kp/128, 0:rows]; everything else -- q's row padding beyond
    Kp (pitch Kp + 16), the scale rows' padding beyond `rows` (pitch rows + 5) and the guards -- is not the
    quantiser's, holds e4m3 NaN codes / E8M0 NaN scales, and must neither change nor reach an output."""
    key = (which, M, N, K)
    if key not in _MXQ:
        a, b, _ = gx.operands("mx", 1, M, N, K)
        src = (a if which == "a" else b)[0]
        rows, kp = src.shape[0], (K + 127) // 128 * 128
        X = gx.Strided(src[None], K + 8, NAN, DEV, dtype=BF)
        Q = gx.Strided(torch.zeros(1, rows, kp, dtype=torch.uint8), kp + 16, E4M3_NAN, DEV)
        Q.view.fill_(E4M3_NAN)
        S = gx.Strided(torch.zeros(1, kp // 128, rows, dtype=torch.int32), rows + 5, E8M0_NAN, DEV)
        S.view.fill_(E8M0_NAN)
        q = ops.mx8_quant(X.view[0], out=ops.MX8(Q.view[0], S.view[0], K))
        torch.cuda.synchronize()
        deq = mx.dequantize(q.q.cpu().numpy(), mx.words_to_e8(q.s.cpu().numpy(), rows))
        assert np.array_equal(deq[:, :K], src.double().numpy()), "the oracle's dequantisation differs from the source"
        assert not q.q[:, K:].any(), "q[:, K:Kp] not zeroed by the quantiser"
        assert Q.padding_intact() and S.padding_intact(), "the quantiser wrote outside q[:, :Kp] / s[:, :rows]"
        _MXQ[key] = (q, Q, S)
    return _MXQ[key]


@pytest.mark.parametrize("cfg", [0, 1, 2, 3])
def test_mx8_kernel(ops, cfg):
    """s2h_mx8_config(cfg): K of MX_K x {264 x 136, 70 x 24} x {bf16, fp32 (beta 0 / 1)} outputs"""
    BM, BN = MX_TILE[cfg]
    tag = gx.make_tag(BM, BN, 2, 2, 2, 128, True, True, mx8=True)
    prev = lib().s2h_mx8_config(cfg)
    try:
        with session(ops) as s:
            for M, N in (gx.SHAPE_RAGGED, gx.SHAPE_PARTIAL):
                for K in MX_K:
                    _, _, acc = gx.operands("mx", 1, M, N, K)
                    (qa, QA, SA), (qb, QB, SB) = _mx_operand(ops, "a", M, N, K), _mx_operand(ops, "b", M, N, K)
                    cold = gx.old_output(1, M, N)
                    for c_dtype, beta in ((BF, 0.0), (F32, 0.0), (F32, 1.0)):
                        what = f"mx8 cfg {cfg} {M}x{N}x{K} {c_dtype} beta {beta}"
                        C = gx.Strided(cold, N + 8, gx.SENT, DEV, dtype=c_dtype)
                        ops.gemm_mx8(qa, qb, C.view[0], beta=beta)
                        s.note(what, tag)
                        s.check(what, C, gx.expected(acc, c_dtype, 1.0, beta, cold))
                    for name, buf in (("q of A", QA), ("s of A", SA), ("q of B", QB), ("s of B", SB)):
                        if not buf.padding_intact():
                            s.fails.append(f"mx8 cfg {cfg} {M}x{N}x{K}: padding of {name} changed")
    finally:
        lib().s2h_mx8_config(prev)
