"""Cases of the GEMM dispatch's host test (test_gemm_plan_host.py): problems, knobs and workspace sizes as the
lines csrc/gemm_plan_host_check.cpp reads, the threshold grid in the fixed order that
tests/golden/gemm_plan_grid.txt records, and the recording's packing.

A problem here is a GEMM over operands with tight pitches and 16-byte aligned bases (layout letters as in
gemm_exact_cases.py: A `n` = [M, K] K-contiguous, `t` = [K, M]; B `t` = [N, K] K-contiguous, `n` = [K, N]), so the
alignment facts follow from the extents: a contiguous extent that is no multiple of 8 (M = 70, K = 1) sends the
problem to the register-staged kernel."""
import base64
import lzma

from sam2_video.kernels import ops

WS = ops.WGRAD_WS_BYTES  # the workspace the training step registers
KNOBS = dict(cfg=0, dbg=0, tiny_cfg=0, w41=1, areg=1, class_cfg=(0, 0, 0, 0, 22, 22), tiny_splitk=0, split_target=768,
             f32_small=1, wg_kmin=ops.WGRAD_KMIN, wg_force_tile=-1, wg_force_splits=0)
LAYOUTS = ("nt", "nn", "tn", "tt")
WGRAD_LAYOUT = "tn"  # both operands row-contiguous over the reduction

GRID_M = (8, 16, 64, 70, 128, 136, 264, 1024, 8184, 8192, 13312, 32768, 65528, 65536, 93184, 131072)
GRID_N = (24, 32, 64, 128, 136, 256, 264, 448, 512, 520, 760, 768, 1016, 1024, 2048)
GRID_K = (1, 8, 64, 72, 120, 128, 136, 200, 248, 256, 264, 320, 448, 512, 520, 1016, 1024, 1032, 2048, 4104, 13312,
          16392, 93184)
# the smaller slice under each non-default knob
SLICE_M = (70, 136, 264, 8192, 65536)
SLICE_N = (24, 136, 512, 1024)
SLICE_K = (8, 72, 264, 1032, 4104)
WG_M = (16, 136, 264, 1024)
WG_N = (64, 136, 512)
WG_K = (520, 1032, 4104, 16392)

PLAN_FIELDS = ("kind", "cfg", "BM", "BN", "WGM", "WGN", "NS", "BK", "splits", "kchunk", "use_ws", "atomic", "zero_c",
               "ws_floats", "wg_tile", "Md", "Nd", "sl", "tag")
KINDS = dict(outer=0, tiny_splitk=1, wgrad=2, glds=3, areg=4, regs=5, f32=6)


def problem(batch, M, N, K, layout, f32_out, epilogue=False, rowsum=False, f32_in=False, beta=0.0, aligned=True,
            pad=None, **over):
    """pad: None = tight pitches; p = pitches rounded up to a multiple of 8, plus p elements"""
    a_kc, b_kc = layout[0] == "n", layout[1] == "t"
    lda, ldb = (K if a_kc else M), (K if b_kc else N)
    if pad is not None:
        lda, ldb = (lda + 7) // 8 * 8 + pad, (ldb + 7) // 8 * 8 + pad
    p = dict(batch=batch, M=M, N=N, K=K, a_kc=a_kc, a_rc=not a_kc or lda == 1, b_kc=b_kc, b_rc=not b_kc or ldb == 1,
                f32_in=f32_in, f32_out=f32_out or f32_in, bias=epilogue, R=False, X=False, cscale=False, dropout=False,
                act=0, beta=beta, rowsum=rowsum, rope=False, lda=lda, ldb=ldb, a16=aligned, b16=aligned,
                sa8=(M * K) % 8 == 0, sb8=(N * K) % 8 == 0, layout=layout)
    assert set(over) <= set(p)
    p.update(over)
    return p


def knobs(**over):
    k = dict(KNOBS)
    k.update(over)
    return k


def case_line(p, k, ws):
    """one line of the host check's input"""
    f = [p["batch"], p["M"], p["N"], p["K"], p["a_kc"], p["a_rc"], p["b_kc"], p["b_rc"], p["f32_in"], p["f32_out"],
         p["bias"], p["R"], p["X"], p["cscale"], p["dropout"], p["act"]]
    g = [p["rowsum"], p["rope"], p["lda"], p["ldb"], p["a16"], p["b16"], p["sa8"], p["sb8"], k["cfg"], k["dbg"],
         k["tiny_cfg"], k["w41"], k["areg"], *k["class_cfg"], k["tiny_splitk"], k["split_target"], k["f32_small"],
         k["wg_kmin"], k["wg_force_tile"], k["wg_force_splits"], ws]
    return " ".join(str(int(x)) for x in f) + f" {float(p['beta'])!r} " + " ".join(str(int(x)) for x in g)


def parse_plan(line):
    return dict(zip(PLAN_FIELDS, (int(x) for x in line.split())))


def _shapes(Ms, Ns, Ks):
    return [(M, N, K) for M in Ms for N in Ns for K in Ks]


def grid():
    """every (problem, knobs, workspace bytes) of the recorded grid, in the recording's order"""
    out = []
    dflt = knobs()
    # default knobs: the whole cross product
    for ws in (WS, 0):
        for epi in (False, True):
            for f32_out in (False, True):
                for batch in (1, 8):
                    for layout in LAYOUTS:
                        for rowsum in ((False, True) if layout == WGRAD_LAYOUT else (False,)):
                            for M, N, K in _shapes(GRID_M, GRID_N, GRID_K):
                                out.append((problem(batch, M, N, K, layout, f32_out, epi, rowsum), dflt, ws))
    sl = [problem(1, M, N, K, layout, f32_out) for f32_out in (False, True) for layout in LAYOUTS
          for M, N, K in _shapes(SLICE_M, SLICE_N, SLICE_K)]
    wg = [problem(1, M, N, K, WGRAD_LAYOUT, True, rowsum=rowsum, beta=beta) for rowsum in (False, True)
          for beta in (0.0, 1.0) for M, N, K in _shapes(WG_M, WG_N, WG_K)]
    for cfg in tuple(range(1, 31)) + (-1,):  # every forced tiling and the register-staged kernel
        out += [(p, knobs(cfg=cfg), WS) for p in sl]
    for tiny in (13, 18, 19):
        out += [(p, knobs(tiny_cfg=tiny), WS) for p in sl if p["M"] <= 136]
    for cls in range(6):
        cc = list(KNOBS["class_cfg"])
        cc[cls] = 9
        out += [(p, knobs(class_cfg=tuple(cc)), WS) for p in sl]
    # tiny split-K on: whole and ragged K chunks, a workspace present, absent and too small for the partials
    tiny = [problem(1, M, N, K, layout, f32_out, epi) for f32_out in (False, True) for epi in (False, True)
            for layout in LAYOUTS for M, N, K in _shapes((8, 70, 104, 128, 136), (24, 256, 520, 1024, 2048),
                                                         (1024, 1032, 2048, 4096, 13312, 16384))]
    for ws in (WS, 0, 65536):
        out += [(p, knobs(tiny_splitk=1), ws) for p in tiny]
    out += [(p, knobs(tiny_splitk=1, tiny_cfg=18), WS) for p in tiny]
    # split targets that give 2 / 4 / 16 splits of the 15 tiles of 264 x 136 (gemm_exact_cases.split_target_for),
    # with the workspace, without it (the atomic form) and with dbg 32 (the atomic form beside a workspace)
    for target in (16, 46, 226):
        for ws, dbg in ((WS, 0), (0, 0), (WS, 32)):
            out += [(p, knobs(split_target=target, dbg=dbg), ws) for p in sl + wg if p["f32_out"]]
            out += [(problem(8, M, N, K, layout, True, beta=beta), knobs(split_target=target, dbg=dbg), ws)
                    for beta in (0.0, 1.0) for layout in LAYOUTS for M, N, K in _shapes((8, 264), (24, 136), (1032, 8200))]
    out += [(p, knobs(dbg=32), WS) for p in sl + wg]
    # reductions long enough for the cap of 256 splits, with the workspace and without
    out += [(problem(batch, M, N, K, layout, True), dflt, ws) for ws in (WS, 0) for batch in (1, 8) for layout in LAYOUTS
            for M, N, K in _shapes((8, 264), (24, 136), (131072, 262144))]
    for tile in range(6):  # s2h_wgrad_force
        for splits in (1, 2, 7, 16):
            out += [(p, knobs(wg_force_tile=tile, wg_force_splits=splits), WS) for p in wg]
    for ws in (4096, 300000):  # a workspace too small for one split of the weight-gradient kernel (of most tiles)
        out += [(p, dflt, ws) for p in wg]
    out += [(p, knobs(wg_kmin=0), WS) for p in wg]  # the kernel and the workspace switched off
    # alignment facts: misaligned bases, row pitches padded to a multiple of 8 (a ragged M or N then fits the
    # weight-gradient kernel's 8-element pieces) and to an odd multiple of 4, batch strides off a multiple of 8
    for kw in (dict(aligned=False), dict(pad=8), dict(pad=4), dict(a16=False), dict(b16=False)):
        out += [(problem(1, M, N, K, layout, f32_out, **kw), dflt, WS) for f32_out in (False, True) for layout in LAYOUTS
                for M, N, K in _shapes(SLICE_M, SLICE_N, SLICE_K)]
        out += [(problem(1, M, N, K, WGRAD_LAYOUT, True, rowsum=rowsum, **kw), dflt, WS) for rowsum in (False, True)
                for M, N, K in _shapes((16, 70, 264), (64, 70, 136), WG_K)]
    for kw in (dict(sa8=False), dict(sb8=False)):
        out += [(problem(batch, M, N, K, layout, False, **kw), dflt, WS) for batch in (1, 8) for layout in LAYOUTS
                for M, N, K in _shapes(SLICE_M, SLICE_N, SLICE_K)]
    # each input of the "plain" predicate on its own, on the outer product (K 1), the split regime and the
    # weight-gradient kernel's shapes
    for kw in (dict(bias=True), dict(R=True), dict(X=True), dict(cscale=True), dict(dropout=True), dict(act=1),
               dict(beta=0.5), dict(beta=1.0), dict(rope=True), dict(rowsum=True)):
        out += [(problem(batch, M, N, K, layout, f32_out, **kw), dflt, WS) for f32_out in (False, True) for batch in (1, 8)
                for layout in LAYOUTS for M, N, K in _shapes((16, 264), (64, 136), (1, 1032, 4104))]
    for small in (1, 0):  # fp32 operands
        out += [(problem(batch, M, N, 72, "nt", True, f32_in=True), knobs(f32_small=small), WS) for batch in (1, 8)
                for M in GRID_M for N in GRID_N]
    return out


# ------------------------------------------------------------------------------------------ the recording
# tests/golden/gemm_plan_grid.txt: `#` comment lines, then the grid's plan lines (one per case, the host check's
# output format) joined by newlines, xz-compressed and base64-encoded in lines of 76 characters
def pack_recording(plan_lines):
    b64 = base64.b64encode(lzma.compress("\n".join(plan_lines).encode(), preset=9 | lzma.PRESET_EXTREME)).decode()
    return "\n".join(b64[i:i + 76] for i in range(0, len(b64), 76)) + "\n"


def unpack_recording(text):
    b64 = "".join(ln for ln in text.split("\n") if not ln.startswith("#"))
    return lzma.decompress(base64.b64decode(b64)).decode().split("\n")
