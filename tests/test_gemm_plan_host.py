"""The GEMM dispatch without a GPU: csrc/gemm_plan.h compiled for the host (csrc/gemm_plan_host_check.cpp: a
stand-alone program, built plain and under the address and undefined-behaviour sanitizers) and run over
  a. the threshold grid of gemm_plan_cases.grid(): every plan equals the one recorded from the dispatch code of the
     commit before the header existed (tests/golden/gemm_plan_grid.txt);
  b. the cases of the exact-integer GPU tests: every plan agrees with the independent Python statement of the rules
     in gemm_exact_cases.py (tags, split plans, the weight-gradient kernel's plans);
  c. the grid again: the invariants a launch relies on hold for every plan."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import gemm_exact_cases as gx
import gemm_plan_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sam2-video-training_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "gemm_plan_grid.txt")
K = C.KINDS


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def host_check(request, tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build csrc/gemm_plan_host_check.cpp")
    exe = tmp_path_factory.mktemp("gemm_plan_host") / f"gemm_plan_host_check_{request.param}"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", *flags, "-I", CSRC,
                    os.path.join(CSRC, "gemm_plan_host_check.cpp"), "-o", str(exe)], check=True)
    return str(exe)


def write_cases(cases, tmp_dir):
    src = os.path.join(tmp_dir, "cases.txt")
    with open(src, "w") as f:
        f.writelines(C.case_line(p, k, ws) + "\n" for p, k, ws in cases)
    return src


def run_host(exe, cases, tmp_dir, src=None):
    """the plan lines of `cases` ((problem, knobs, workspace bytes) each; src: their file, when already written)"""
    src, dst = src or write_cases(cases, tmp_dir), os.path.join(tmp_dir, f"plans_{os.path.basename(exe)}.txt")
    subprocess.run([exe, src, dst], check=True, timeout=300)
    with open(dst) as f:
        lines = f.read().split("\n")
    assert lines.pop() == "" and len(lines) == len(cases)
    return lines


@pytest.fixture(scope="module")
def grid():
    return C.grid()


@pytest.fixture(scope="module")
def grid_file(grid, tmp_path_factory):
    return write_cases(grid, str(tmp_path_factory.mktemp("gemm_plan_grid")))


@pytest.fixture(scope="module")
def grid_plans(host_check, grid, grid_file):
    return run_host(host_check, grid, os.path.dirname(grid_file), grid_file)


def describe(case):
    p, k, ws = case
    diff = {n: v for n, v in k.items() if v != C.KNOBS[n]}
    return (f"{p['batch']}x{p['M']}x{p['N']}x{p['K']} {p['layout']} {'fp32' if p['f32_out'] else 'bf16'} out, "
            f"problem {p}, knobs {diff}, workspace {ws}")


# ------------------------------------------------------------------------------------------ a. the recording
def test_grid_is_the_cross_product_the_recording_claims(grid):
    n_shapes = len(C.GRID_M) * len(C.GRID_N) * len(C.GRID_K)
    # workspace x epilogue x output x batch x (four layouts + the weight-gradient layout with row sums)
    head = grid[:2 * 2 * 2 * 2 * 5 * n_shapes]
    assert all(k == C.KNOBS for _, k, _ in head)
    assert {ws for _, _, ws in head} == {C.WS, 0} and {p["batch"] for p, _, _ in head} == {1, 8}
    assert {(p["M"], p["N"], p["K"]) for p, _, _ in head} == {(M, N, Kk) for M in C.GRID_M for N in C.GRID_N
                                                               for Kk in C.GRID_K}
    assert {p["layout"] for p, _, _ in head if p["rowsum"]} == {C.WGRAD_LAYOUT}
    tail = grid[80 * n_shapes:]
    assert {k["cfg"] for _, k, _ in tail} >= set(gx.FORCED_NUMBERS)
    assert {k["tiny_cfg"] for _, k, _ in tail} >= {13, 18, 19}
    assert {k["class_cfg"] for _, k, _ in tail} >= {tuple(9 if i == c else v for i, v in enumerate(C.KNOBS["class_cfg"]))
                                                    for c in range(6)}
    assert {(k["wg_force_tile"], k["wg_force_splits"]) for _, k, _ in tail} >= {(t, s) for t in gx.WG_TILES
                                                                                for s in gx.WG_SPLITS}
    assert any(k["tiny_splitk"] for _, k, _ in tail) and any(k["dbg"] == 32 for _, k, _ in tail)
    assert {k["split_target"] for _, k, _ in tail} >= {16, 46, 226}
    # the recording holds every kind of plan, and split plans in all three forms
    with open(GOLDEN) as f:
        want = [C.parse_plan(ln) for ln in set(C.unpack_recording(f.read()))]
    assert {p["kind"] for p in want} == set(K.values())
    assert any(p["use_ws"] and p["kind"] == K["glds"] for p in want) and any(p["atomic"] and p["zero_c"] for p in want)
    assert any(p["atomic"] and not p["zero_c"] for p in want) and any(p["splits"] == 256 for p in want)


def test_plans_equal_the_recorded_dispatch(grid, grid_plans):
    with open(GOLDEN) as f:
        want = C.unpack_recording(f.read())
    assert len(want) == len(grid)
    bad = [i for i, (g, w) in enumerate(zip(grid_plans, want)) if g != w]
    assert not bad, (f"{len(bad)} of {len(grid)} plans differ from the recording; first: {describe(grid[bad[0]])}: "
                     f"got {C.parse_plan(grid_plans[bad[0]])} want {C.parse_plan(want[bad[0]])}")


# ------------------------------------------------------------------------------------------ b. the Python model
# test_gemm_exact_gpu.py test_generic_split_k's cases: name -> (batch, M, N, layout, forced cfg), and its (K, splits)
SPLIT_CASES = {"batch 3": (3, 264, 136, "tn", 0), "M < 16": (1, 8, 136, "tn", 0), "N < 64": (1, 264, 24, "tn", 0),
               "forced 128x64": (1, 264, 136, "tn", 7), "forced 64x64 K-contiguous": (1, 264, 136, "nt", 1)}
SPLIT_K = ((1032, 2), (2056, 4), (8200, 16))


def _split_tile(M, cfg):
    n = cfg or (18 if M <= 128 else 1)
    return n, gx.FORCED[n][1], gx.FORCED[n][2]


def model_cases():
    """(what, case, check) with check(plan) -> None or a message"""
    out = []
    F32 = gx.F32

    def add(what, p, k, ws, check):
        out.append((what, (p, k, ws), check))

    def tag_is(tag, **fields):
        def check(pl):
            if pl["tag"] != tag:
                return f"tag {gx.decode_tag(pl['tag'])} want {gx.decode_tag(tag)}"
            bad = {n: (pl[n], v) for n, v in fields.items() if pl[n] != v}
            return f"(got, want) {bad}" if bad else None
        return check

    aligned = dict(pad=8, sa8=True, sb8=True)  # the GPU tests' operands: pitches and batch strides multiples of 8
    for rule, (batch, M, N, Kk, layout, dt, cfg, tiny) in gx.RULES.items():
        add(f"rule {rule}", C.problem(batch, M, N, Kk, layout, dt == F32, **aligned), C.knobs(tiny_cfg=tiny), C.WS,
            tag_is(gx.cfg_tag(cfg, layout), cfg=cfg))
    tag9 = gx.cfg_tag(9, "nt")
    for cls, (inside, outside) in gx.CLASSES.items():
        cc = tuple(9 if i == cls else v for i, v in enumerate(C.KNOBS["class_cfg"]))
        add(f"class {cls} inside", C.problem(1, *inside, "nt", False, **aligned), C.knobs(class_cfg=cc), C.WS,
            tag_is(tag9, cfg=9))
        for shp in (outside, (128,) + inside[1:]):
            add(f"class {cls} outside {shp}", C.problem(1, *shp, "nt", False, **aligned), C.knobs(class_cfg=cc), C.WS,
                lambda pl: None if pl["tag"] not in (tag9, 0) else "runs on the class's configuration")
    for cfg in gx.FORCED_NUMBERS:
        for M, N in (gx.SHAPE_RAGGED, gx.SHAPE_PARTIAL):
            for layout in gx.LAYOUTS:
                for Kk in gx.K_LIST:
                    for batch in (1, 3):
                        for f32_out in (False, True):
                            tag, own = gx.forced_tag(cfg, M, N, Kk, layout, batch)
                            add(f"forced {cfg} {batch}x{M}x{N}x{Kk} {layout}", C.problem(batch, M, N, Kk, layout, f32_out, **aligned),
                                C.knobs(cfg=cfg), C.WS, tag_is(tag, cfg=99 if cfg < 0 else cfg) if own else tag_is(tag))
                    tag, _ = gx.forced_tag(cfg, M, N, Kk, layout, aligned=False)
                    add(f"forced {cfg} {M}x{N}x{Kk} {layout} base + 1", C.problem(1, M, N, Kk, layout, False, pad=8, a16=False),
                        C.knobs(cfg=cfg), C.WS, tag_is(tag, kind=K["regs"]))
    # the register-staged kernel (test_register_staged): forced, and with nothing forced a misaligned base, row
    # pitches that are no multiple of 8, K = 0
    for M, N in (gx.SHAPE_RAGGED, gx.SHAPE_PARTIAL):
        for layout in gx.LAYOUTS:
            for Kk in (1, 5, 67, 515):
                add(f"regs {M}x{N}x{Kk} {layout}", C.problem(1, M, N, Kk, layout, True, beta=1.0, pad=8), C.knobs(cfg=-1), C.WS,
                    tag_is(gx.regs_tag(M, N, Kk, layout), kind=K["regs"]))
    M, N = gx.SHAPE_RAGGED
    for layout in gx.LAYOUTS:
        for Kk in (72, 520):
            for kw in (dict(pad=8, a16=False), dict(pad=3), dict(pad=5)):
                add(f"regs {kw} {M}x{N}x{Kk} {layout}", C.problem(1, M, N, Kk, layout, False, **kw), C.knobs(), C.WS,
                    tag_is(gx.regs_tag(M, N, Kk, layout), kind=K["regs"]))
        add(f"regs K 0 {layout}", C.problem(1, M, N, 0, layout, True, pad=8), C.knobs(), C.WS,
            tag_is(gx.regs_tag(M, N, 0, layout), kind=K["regs"], splits=1))
    # generic split-K (test_generic_split_k, test_generic_split_k_rowsum): workspace and atomic form
    for atomic in (0, 1):
        split_cases = [(name, *v, False) for name, v in SPLIT_CASES.items()]
        split_cases += [(f"rowsum {Nl}x{Kl}", 1, Nl, Kl, "tn", 0, True) for Nl, Kl in ((8, 136), (264, 24))]
        for name, batch, M, N, layout, cfg, rowsum in split_cases:
            n, BM, BN = _split_tile(M, cfg)
            for Kk, want in SPLIT_K:
                target = gx.split_target_for(M, N, Kk, batch, BM, BN, want)
                splits, kchunk, per = gx.plan_splits(M, N, Kk, batch, BM, BN, target, rowsum=rowsum)
                assert splits >= 2
                for beta in (0.0, 1.0):
                    add(f"split {name} K {Kk} x{splits} atomic {atomic} beta {beta}",
                        C.problem(batch, M, N, Kk, layout, True, rowsum=rowsum, beta=beta, **aligned),
                        C.knobs(cfg=cfg, dbg=32 * atomic, split_target=target), C.WS,
                        tag_is(gx.cfg_tag(n, layout), cfg=n, splits=splits, kchunk=kchunk, use_ws=1 - atomic, atomic=atomic,
                               zero_c=int(atomic and beta == 0.0), ws_floats=0 if atomic else splits * per))
    # the deterministic weight-gradient kernel (test_wgrad_det_forced): wg_plan, wg_smax, wg_k_last8, wg_k_fewer
    M, N = gx.SHAPE_RAGGED
    combos = [(Kk, sp) for Kk in gx.WG_K for sp in gx.WG_SPLITS] + [gx.wg_k_last8(), gx.wg_k_fewer()]
    for tile, (BM, BN, _, _, _) in gx.WG_TILES.items():
        ntm, ntn = (M + BM - 1) // BM, (N + BN - 1) // BN
        for Kk, sp in combos:
            if sp > gx.wg_smax(Kk):
                continue  # (beyond the cost model's range, which the Python statement covers)
            splits, kchunk, _ = gx.wg_plan(Kk, sp)
            for rowsum in (False, True):
                n = splits * ntm * ntn * BM * BN + (splits * ntm * BM if rowsum else 0)
                add(f"wgrad tile {tile} K {Kk} forced {sp}", C.problem(1, M, N, Kk, "tn", True, rowsum=rowsum, pad=8),
                    C.knobs(wg_force_tile=tile, wg_force_splits=sp), C.WS,
                    tag_is(gx.wg_tag(tile), kind=K["wgrad"], wg_tile=tile, splits=splits, kchunk=kchunk, use_ws=1, ws_floats=n,
                           Md=(M + 7) // 8 * 8, Nd=(N + 7) // 8 * 8))
    for Kk in gx.WG_K + (gx.wg_k_last8()[0], 20000, 93184):  # the cost model's own split count stays within wg_smax
        add(f"wgrad K {Kk} unforced", C.problem(1, M, N, Kk, "tn", True, pad=8), C.knobs(), C.WS,
            lambda pl, Kk=Kk: None if pl["kind"] == K["wgrad"] and 1 <= pl["splits"] <= gx.wg_smax(Kk) else
            f"kind {pl['kind']} splits {pl['splits']} beyond wg_smax {gx.wg_smax(Kk)}")
    add("wgrad 4099x130x77 (pitches no multiple of 8)", C.problem(1, 130, 77, 4099, "tn", True), C.knobs(), C.WS,
        tag_is(gx.regs_tag(130, 77, 4099, "tn"), kind=K["regs"]))
    return out


def test_plans_agree_with_the_python_statement_of_the_rules(host_check, tmp_path):
    cases = model_cases()
    assert len(cases) > 5000
    plans = [C.parse_plan(ln) for ln in run_host(host_check, [c for _, c, _ in cases], str(tmp_path))]
    bad = [(what, msg, describe(case)) for (what, case, check), pl in zip(cases, plans) for msg in [check(pl)] if msg]
    assert not bad, (len(bad), bad[:5])


# ------------------------------------------------------------------------------------------ c. invariants
def _column(grid, name, src=0):
    return np.asarray([c[src][name] for c in grid], dtype=np.float64 if name == "beta" else np.int64)


def test_every_plan_keeps_the_launch_invariants(grid, grid_plans):
    pl = dict(zip(C.PLAN_FIELDS, np.asarray([ln.split() for ln in grid_plans], dtype=np.int64).T))
    p = {n: _column(grid, n) for n in ("batch", "M", "N", "K", "a_kc", "b_kc", "f32_in", "f32_out", "bias", "R", "X", "cscale",
                                      "dropout", "act", "beta", "rowsum", "rope", "lda", "ldb", "a16", "b16", "sa8", "sb8")}
    ws = np.asarray([c[2] for c in grid], dtype=np.int64)
    kmin = _column(grid, "wg_kmin", 1)
    kind, splits, kchunk = pl["kind"], pl["splits"], pl["kchunk"]
    bf16_gemm = kind != K["f32"]

    def holds(what, cond):
        bad = np.nonzero(~cond)[0]
        assert bad.size == 0, (what, bad.size, describe(grid[bad[0]]), C.parse_plan(grid_plans[bad[0]]))

    # the K chunks: whole 64-deep stages when K is split, and exactly `splits` non-empty chunks covering K
    holds("kchunk of a split plan is a multiple of 64", (splits == 1) | (kchunk % 64 == 0))
    holds("the chunks cover K, none empty", ((splits - 1) * kchunk < p["K"]) & (p["K"] <= splits * kchunk))
    holds("1 <= splits <= 256", (splits >= 1) & (splits <= 256))
    # the workspace: needed only by a plan that uses it, and never more than the registered capacity
    cap = np.where(kmin > 0, ws, 0)
    holds("workspace need within capacity", np.where(pl["use_ws"] == 1, (pl["ws_floats"] > 0) & (pl["ws_floats"] * 4 <= cap),
                                                     pl["ws_floats"] == 0))
    holds("workspace or atomics, not both", (pl["use_ws"] + pl["atomic"] <= 1) & ((splits == 1) | (pl["use_ws"] + pl["atomic"] == 1)))
    holds("C zeroed only for the atomic form at beta 0", pl["zero_c"] == (pl["atomic"] & (p["beta"] == 0.0)))
    # a split plan only on a plain fp32-output problem (tiny split-K, the one exception, runs the epilogue in its
    # second launch over the summed partials: bf16 output, batch 1)
    plain = ((p["f32_out"] == 1) & (p["bias"] + p["R"] + p["X"] + p["cscale"] + p["dropout"] + p["act"] == 0) &
             ((p["beta"] == 0.0) | (p["beta"] == 1.0)))
    tiny = kind == K["tiny_splitk"]
    holds("split only when plain with an fp32 output", (splits == 1) | tiny | plain)
    holds("tiny split-K: bf16 output, batch 1, M <= 128, whole chunks < 1024",
          ~tiny | ((p["f32_out"] == 0) & (p["batch"] == 1) & (p["M"] <= 128) & (splits * kchunk == p["K"]) & (kchunk < 1024) &
                   (splits >= 4)))
    # the LDS-DMA path's requirements, stated from the kernels' addressing (gemm_bf16.h): 16-B pieces from aligned
    # bases and pitches, whole 8-element pieces along the contiguous extent, 32-bit element offsets
    aext, bext = np.where(p["a_kc"] == 1, p["K"], p["M"]), np.where(p["b_kc"] == 1, p["K"], p["N"])
    aspan = np.where(p["a_kc"] == 1, p["M"], p["K"]) * p["lda"]
    bspan = np.where(p["b_kc"] == 1, p["N"], p["K"]) * p["ldb"]
    glds = ((p["a16"] == 1) & (p["b16"] == 1) & (p["lda"] % 8 == 0) & (p["ldb"] % 8 == 0) & (aext % 8 == 0) & (bext % 8 == 0) &
            ((p["batch"] == 1) | ((p["sa8"] == 1) & (p["sb8"] == 1))) & (p["K"] > 0) & (aspan < 2 ** 31) & (bspan < 2 ** 31))
    holds("an LDS-DMA plan only on operands it can address", ~((kind == K["glds"]) | tiny) | glds)
    holds("aligned operands never take the register-staged kernel unless forced",
          ~(bf16_gemm & (kind == K["regs"]) & glds) | (_column(grid, "cfg", 1) < 0))
    areg = kind == K["areg"]
    holds("A in registers: K-contiguous aligned A, K <= 256 in 8-element pieces, no row sums, no split",
          ~areg | ((p["a_kc"] == 1) & (p["K"] <= 256) & (p["K"] > 0) & (p["K"] % 8 == 0) & (p["a16"] == 1) & (p["lda"] % 8 == 0) &
                   (p["sa8"] == 1) & (p["rowsum"] == 0) & (splits == 1) & glds))
    wg = kind == K["wgrad"]
    holds("weight-gradient kernel: batch 1, both operands row-contiguous, plain, aligned, padded extents inside the pitch",
          ~wg | ((p["batch"] == 1) & (p["a_kc"] == 0) & (p["b_kc"] == 0) & plain & (p["rope"] == 0) & (p["a16"] == 1) &
                 (p["b16"] == 1) & (p["lda"] % 8 == 0) & (p["ldb"] % 8 == 0) & (pl["Md"] % 8 == 0) & (pl["Nd"] % 8 == 0) &
                 (pl["Md"] >= p["M"]) & (pl["Md"] < p["M"] + 8) & (pl["Nd"] >= p["N"]) & (pl["Nd"] < p["N"] + 8) &
                 (pl["Md"] <= p["lda"]) & (pl["Nd"] <= p["ldb"]) & (pl["use_ws"] == 1) & (p["K"] * p["lda"] < 2 ** 31) &
                 (p["K"] * p["ldb"] < 2 ** 31)))
    holds("reduce slices: a power of two <= min(16, splits)",
          ~wg | ((pl["sl"] >= 1) & (pl["sl"] <= 16) & (pl["sl"] <= splits) & ((pl["sl"] & (pl["sl"] - 1)) == 0)))
    holds("the outer-product kernel: K 1, no epilogue, beta 0", ~(kind == K["outer"]) | (
        (p["K"] == 1) & (p["beta"] == 0.0) & (p["bias"] + p["R"] + p["X"] + p["cscale"] + p["dropout"] + p["act"] + p["rowsum"] +
                                              p["rope"] == 0)))
    holds("fp32 operands take the fp32 kernel, nothing else does", (kind == K["f32"]) == (p["f32_in"] == 1))
    holds("a tiling number with every tiled plan", np.where((kind == K["glds"]) | areg | tiny, (pl["cfg"] >= 1) & (pl["cfg"] <= 30),
                                                            np.where(kind == K["regs"], pl["cfg"] == 99, pl["cfg"] == 0)))


def test_host_check_refuses_malformed_cases(host_check, tmp_path):
    good = C.case_line(C.problem(1, 264, 136, 72, "nt", False), C.knobs(), C.WS)
    for text in (good.rsplit(" ", 1)[0], good.replace("264", "0", 1), "1 264 136 72 2 " + good.split(" ", 5)[5]):
        src, dst = tmp_path / "in.txt", tmp_path / "out.txt"
        src.write_text(text + "\n")
        assert subprocess.run([host_check, str(src), str(dst)], timeout=60).returncode == 3, text
