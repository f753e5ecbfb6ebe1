"""Every softmax implementation of the attention kernels (csrc/flash.hip, flash_bwd.hip, attention.hip)
on the structured inputs of attn_cases.py -- peaked rows, key ramps that move the row maximum on every
tile, spikes whose neighbours underflow to exactly 0, all scores offset by +-60 nats -- against the float64
reference on the same rounded inputs.  test_attention_conditioning_host.py proves on the CPU that these
inputs make the flash forward rescale after tile 0 (randn inputs never do), and that a forward without
the rescale misses the tolerance used here by more than 10x.

o is compared per query row (a flat row cannot hide behind a peaked one), the LSE absolutely (a bound
relative to max |lse| would tolerate 0.2 nats at |lse| = 200), the gradients per tensor.

The tolerances are the issue's: tol_o 2e-2 is the sibling tests' value and about 5x the torch model of the
flash forward (3.7e-3); the LSE's absolute 1e-3 is about 40x that model (2.5e-5; an fp32 ulp at 200 log2
units is 1.5e-5); the gradient bounds 4e-2 (flash) and 6e-2 (tile kernels) are the sibling values, about
2x the torch model of the bf16 backward on unshifted cases (2.1e-2); the fp32 bounds are a few fp32 ulps
of a 200-log2-unit exponent.  Every case asserts the kernels it is named for: the flash eligibility as the
library reports it under the case's switches, and attention.hip's dispatch on the shape."""
import gc
from contextlib import contextmanager

import pytest
import torch

import attn_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (tol_o per row, lse absolute, gradients per tensor)
TOL_FLASH = (2e-2, 1e-3, 4e-2)  # emulated: o 3.7e-3, lse 2.5e-5 (test_attention_conditioning_host.py)
TOL_BF16 = (2e-2, 1e-3, 6e-2)   # whole-window, generic, few-query and few-key kernels in bf16
TOL_FP32 = (1e-4, 2e-4, 3e-4)   # a few fp32 ulps of a 200-log2-unit exponent (ulp 1.5e-5)


def _ops():
    from sam2_video.kernels import ops
    return ops


def _lib():
    from sam2_video.kernels._lib import lib
    return lib()


@contextmanager
def _knobs(config=1, sets=None, v2=0, win=1):
    """s2h_attn_config (bit 0 flash on, bit 6 the V-fold's 2-stage ring, bits 8+ the key split's workgroup
    target), s2h_flash_fwd_sets, s2h_flash_variant2 and s2h_attn_win for one launch, restored after"""
    lib = _lib()
    p_cfg = lib.s2h_attn_config(config)
    p_sets = lib.s2h_flash_fwd_sets(-1 if sets is None else sets)
    p_v2 = lib.s2h_flash_variant2(v2)
    p_win = lib.s2h_attn_win(win)
    try:
        yield
    finally:
        lib.s2h_attn_win(p_win)
        lib.s2h_flash_variant2(p_v2)
        lib.s2h_flash_fwd_sets(p_sets)
        lib.s2h_attn_config(p_cfg)


def plan_splits(BH, Lq, Lk, qs, target):
    """flash_plan (csrc/flash.hip): key splits of a forward with qs 16-query sets per wave"""
    base = -(-Lq // (128 * qs)) * BH
    ntiles = -(-Lk // 64)
    s = max(1, min((target or 256) // base, ntiles // 2))
    tps = -(-ntiles // s)
    return -(-ntiles // tps)


class Path:
    """route: the kernels the case is named for, "forward dq dkv" (flash: all three on flash.hip / flash_bwd.hip)"""

    def __init__(self, name, shape, dtype=torch.bfloat16, tol=TOL_BF16, kind="attn", splits=None, qs=1,
                 route="flash flash flash", **knobs):
        self.name, self.shape, self.dtype, self.tol, self.kind = name, shape, dtype, tol, kind
        self.splits, self.qs, self.knobs, self.route = splits, qs, knobs, tuple(route.split())

    def __repr__(self):
        return self.name


def _flash_paths():
    out = []
    for shape in [(1, 2, 130, 300, 56), (1, 2, 130, 300, 72), (1, 2, 130, 300, 256), (1, 2, 130, 450, 72)]:
        B, H, Lq, Lk, D = shape
        many = 2 if Lk == 300 else 4  # the SPL = 2 combine / the general vectorised one
        if D == 256:  # one query set per wave whatever the switch says
            forms = [("one", 0x11, 1, 0), ("split", 0x11, 0, 0), ("split-rowcombine", 0x11, 0, 16)]
        else:
            forms = [("sets1-one", 0x11, 1, 0), ("sets2-one", 0x22, 1, 0), ("sets2-one-ring3", 0x22, 1, 4),
                     ("sets1-split", 0x11, 0, 0), ("sets2-split", 0x22, 0, 0), ("sets1-split-rowcombine", 0x11, 0, 16),
                     ("sets2-split-rowcombine-ring3", 0x22, 0, 4 | 16)]
        for tag, sets, target, v2 in forms:
            out.append(Path(f"flash-{Lk}x{D}-{tag}", shape, tol=TOL_FLASH, splits=1 if target == 1 else many,
                            qs=2 if sets == 0x22 and D <= 128 else 1, config=1 | (target << 8), sets=sets, v2=v2))
    return out


def _vfold_paths():
    out = []
    for B, Lq, Lk in [(2, 130, 300), (2, 130, 450)]:
        many = 2 if Lk == 300 else 4
        for tag, ring2, sets, target, v2 in [("ring3-sets2-split", 0, 0x22, 0, 0), ("ring3-sets1-one", 0, 0x11, 1, 0),
                                             ("ring2-sets2-one", 64, 0x22, 1, 0), ("ring2-sets1-split", 64, 0x11, 0, 0),
                                             ("ring3-sets2-split-rowcombine", 0, 0x22, 0, 16)]:
            out.append(Path(f"vfold-{Lk}-{tag}", (B, 1, Lq, Lk, 256), tol=TOL_FLASH, kind="vfold",
                            splits=1 if target == 1 else many, qs=2 if sets == 0x22 else 1,
                            config=1 | ring2 | (target << 8), sets=sets, v2=v2))
    return out


def _tile_paths():
    f32, bf = torch.float32, torch.bfloat16
    G = "generic generic generic"
    out = []
    for shape in [(1, 2, 70, 300, 32), (1, 2, 70, 300, 96), (1, 1, 70, 130, 256)]:  # Lq < 128: never flash
        out.append(Path("generic-fp32-%dx%dx%d" % shape[2:], shape, f32, TOL_FP32, route=G))
        out.append(Path("generic-bf16-%dx%dx%d" % shape[2:], shape, bf, TOL_BF16, route=G))
    out.append(Path("generic-bf16-130x300x56-flash-off", (1, 2, 130, 300, 56), bf, TOL_BF16, route=G, config=0))
    # few queries: the cross-wave merge (16-wave bf16 form at head dim 16: 11 of its waves own no key tile)
    out.append(Path("fewq-bf16-8x300x16", (2, 2, 8, 300, 16), bf, TOL_BF16, route="fewq fewq fewq_dkv"))
    out.append(Path("fewq-fp32-8x300x16", (2, 2, 8, 300, 16), f32, TOL_FP32, route="fewq fewq generic"))
    out.append(Path("fewq-bf16-16x1000x64", (1, 2, 16, 1000, 64), bf, TOL_BF16, route="fewq fewq fewq_dkv"))
    # few keys: forward on the whole-window kernel (win 1) or the tile kernel (win 0), few-key backward (its dq
    # on attn_fewk_dq_kernel with win 1).  300 x 16 x 64 is flash-eligible: the flash switch is off for it
    for shape, cfg in [((2, 2, 300, 8, 16), 1), ((1, 2, 300, 16, 64), 0)]:
        out.append(Path("fewk-bf16-%dx%dx%d-win1" % shape[2:], shape, bf, TOL_BF16, route="win fewk_dq fewk", win=1, config=cfg))
        out.append(Path("fewk-bf16-%dx%dx%d-win0" % shape[2:], shape, bf, TOL_BF16, route="generic generic fewk", win=0,
                        config=cfg))
    out.append(Path("fewk-fp32-300x8x16", (2, 2, 300, 8, 16), f32, TOL_FP32, route="generic generic fewk"))
    # whole windows (attn_win_*) against the tile kernels on the same single key tile.  130 x 40 x 64 is
    # flash-eligible too (switched off): its forward runs attn_win_fwd over three query tiles, its backward
    # (more than 64 queries) the tile kernels
    for shape, cfg, r1 in [((3, 2, 49, 49, 56), 1, "win win win"), ((2, 2, 130, 40, 64), 0, "win generic generic"),
                           ((4, 2, 8, 20, 32), 1, "win win win"), ((4, 2, 8, 50, 32), 1, "win win win")]:
        out.append(Path("win-bf16-%dx%dx%d-win1" % shape[2:], shape, bf, TOL_BF16, route=r1, win=1, config=cfg))
        out.append(Path("win-bf16-%dx%dx%d-win0" % shape[2:], shape, bf, TOL_BF16, route=G, win=0, config=cfg))
    # the two flash-eligible shapes above with the switch on: the flash kernels on a single key tile
    for shape in [(1, 2, 300, 16, 64), (2, 2, 130, 40, 64)]:
        out.append(Path("flash-onetile-%dx%dx%d" % shape[2:], shape, bf, TOL_FLASH, splits=1, qs=2, config=1, sets=0x22))
    return out


PATHS = _flash_paths() + _vfold_paths() + _tile_paths()
_REF, _RUN = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _release_caches():
    """the shared references and runs (a few hundred MB of host memory) go when the module is done: the
    tests that follow in the same process, and the loader workers they fork, do not carry them"""
    yield
    _REF.clear()
    _RUN.clear()
    gc.collect()


def _seed(shape):
    return sum(x * 131 ** i for i, x in enumerate(shape)) % 100003


def _ref(path, profile, shift):
    """inputs and the float64 reference of one case, shared by every path on that shape and dtype"""
    B, H, Lq, Lk, D = path.shape
    Dv = 64 if path.kind == "vfold" else D
    key = (path.shape, Dv, path.dtype, profile, shift)
    if key not in _REF:
        q, k, v = C.make_qkv(B, H, Lq, Lk, D, profile, shift, Dv=Dv, seed=_seed(path.shape), dtype=path.dtype)
        do = None
        if path.kind == "attn":
            do = torch.randn(B, Lq, H, D, generator=torch.Generator().manual_seed(7)).to(path.dtype)
        ref = C.reference(q, k, v, D ** -0.5, do=do)
        del ref["s"]  # the score matrix is the largest entry and no check here reads it
        _REF[key] = (q, k, v, do, ref)
    return _REF[key]


def _check_plan(path):
    """the split count the case is named for, as ops sizes the workspace from it (flash_plan's formula): a
    change of plan cannot quietly turn a combine case into a one-split case"""
    if path.splits is None:
        return
    ops, lib = _ops(), _lib()
    B, H, Lq, Lk, D = path.shape
    target = path.knobs["config"] >> 8
    assert plan_splits(B * H, Lq, Lk, path.qs, target) == path.splits
    if path.kind == "vfold":
        nws, per = lib.s2h_attn_fwd_vfold_ws_bytes(B, Lq, Lk), B * Lq * (64 + 4) * 4
    else:
        dp = 64 if D <= 64 else 128 if D <= 128 else 256
        nws, per = lib.s2h_attn_fwd_ws_bytes(ops.BF16, B, H, Lq, Lk, D), B * H * Lq * (dp + 2) * 4
    assert nws == (path.splits * per if path.splits > 1 else 0), (nws, per, path.splits)


def _route(path):
    """the kernels a case runs: flash where the library says so under the case's switches (s2h_attn_fwd and
    s2h_attn_bwd ask that first), else attention.hip's dispatch (attn_win_ok, attn_fewq, attn_fewk and the
    bf16 single-tile dq / dkv kernels), without dropout"""
    ops = _ops()
    B, H, Lq, Lk, D = path.shape
    bf = path.dtype == torch.bfloat16
    if _lib().s2h_flash_bwd_ok(ops.BF16 if bf else ops.F32, Lq, D):
        return ("flash", "flash", "flash")
    win = bool(path.knobs.get("win", 1)) and bf and D <= 64
    fewq, fewk = Lq <= 16 and Lk > 128 and D <= 64, Lk <= 16 and Lq > 128 and D <= 64
    fwd = "win" if win and Lk <= 64 else "fewq" if fewq else "generic"
    if win and Lq <= 64 and Lk <= 64:
        return (fwd, "win", "win")
    dq = "fewq" if fewq else "fewk_dq" if win and Lk <= 16 else "generic"
    dkv = "fewk" if fewk else "fewq_dkv" if win and Lq <= 16 else "generic"
    return (fwd, dq, dkv)


def test_every_kernel_family_is_named_by_a_case():
    """the cases' declared routes cover each softmax implementation at each head-dim image it is built for"""
    have = {(r, 32 if p.shape[4] <= 32 else 64 if p.shape[4] <= 64 else 128, p.dtype == torch.bfloat16)
            for p in PATHS for r in zip(("fwd", "dq", "dkv"), p.route)}
    for want in [(("fwd", "win"), 32, True), (("fwd", "win"), 64, True), (("dq", "win"), 32, True), (("dq", "win"), 64, True),
                 (("fwd", "fewq"), 32, True), (("fwd", "fewq"), 64, True), (("fwd", "fewq"), 32, False),
                 (("dkv", "fewq_dkv"), 32, True), (("dkv", "fewq_dkv"), 64, True),
                 (("dkv", "fewk"), 32, True), (("dkv", "fewk"), 64, True), (("dkv", "fewk"), 32, False),
                 (("dq", "fewk_dq"), 32, True), (("dq", "fewk_dq"), 64, True),
                 (("fwd", "generic"), 32, True), (("fwd", "generic"), 64, True), (("fwd", "generic"), 128, True),
                 (("fwd", "generic"), 32, False), (("fwd", "flash"), 64, True), (("fwd", "flash"), 128, True)]:
        assert want in have, want
    # attn_win_fwd over several query tiles (grid.y > 1)
    assert any(p.route[0] == "win" and p.shape[2] > 64 for p in PATHS)


def _run(path, profile, shift):
    """the kernels' outputs of one case on the CPU, NaN-filled before the launch"""
    key = (path.name, profile, shift)
    if key in _RUN:
        return _RUN[key]
    ops = _ops()
    q, k, v, do, _ = _ref(path, profile, shift)
    B, H, Lq, Lk, D = path.shape
    q, k, v = q.to(DEV), k.to(DEV), v.to(DEV)
    nan = float("nan")
    lse = torch.full((B, H, Lq), nan, device=DEV)
    with _knobs(**path.knobs):
        _check_plan(path)
        assert _route(path) == path.route, (path.name, _route(path), path.route)
        if path.kind == "vfold":
            u = torch.full((B, Lq, 1, 72), nan, device=DEV, dtype=path.dtype)
            ops.attn_fwd_vfold(q, k, v, u, lse, D ** -0.5)
            res = {"u": u, "lse": lse}
        else:
            do = do.to(DEV)
            o = torch.full_like(q, nan)
            ops.attn_fwd(q, k, v, o, lse, D ** -0.5)
            dq, dk, dv = (torch.full_like(t, nan) for t in (q, k, v))
            ops.attn_bwd(q, k, v, o, do, lse, dq, dk, dv, D ** -0.5)
            res = {"o": o, "lse": lse, "dq": dq, "dk": dk, "dv": dv}
        torch.cuda.synchronize()
    _RUN[key] = {n: t.cpu() for n, t in res.items()}
    return _RUN[key]


@pytest.mark.parametrize("shift", C.SHIFTS, ids=lambda s: "shift%+d" % s)
@pytest.mark.parametrize("profile", C.PROFILES)
@pytest.mark.parametrize("path", PATHS, ids=repr)
def test_attention_on_structured_scores(path, profile, shift):
    tol_o, tol_lse, tol_g = path.tol
    ref = _ref(path, profile, shift)[4]
    got = _run(path, profile, shift)
    for n, t in got.items():
        assert torch.isfinite(t.float()).all(), f"{n}: NaN or infinity"
    o = got["u"][..., :64] if path.kind == "vfold" else got["o"]
    errs = {"o": C.row_err(o, ref["o"]).max().item(), "lse": (got["lse"].double() - ref["lse"]).abs().max().item()}
    fails = []
    if errs["o"] > tol_o:
        fails.append("o")
    if errs["lse"] > tol_lse:
        fails.append("lse")
    if path.kind == "vfold":  # u' = [P mem | rowsum(P) = 1 | 0 x 7]
        assert torch.all(got["u"][..., 64] == 1) and torch.all(got["u"][..., 65:] == 0)
    else:
        for n in ("dq", "dk", "dv"):
            errs[n] = C.tensor_err(got[n], ref[n])
            # shifted bf16 cases: the rounding of dS times the enlarged keys alone reaches 2.5e-2 in dq
            if errs[n] > tol_g and not (n == "dq" and shift and path.dtype == torch.bfloat16):
                fails.append(n)
    if shift:  # the offset moves the LSE and nothing else
        ref0, got0 = _ref(path, profile, 0.0)[4], _run(path, profile, 0.0)
        o0 = got0["u"][..., :64] if path.kind == "vfold" else got0["o"]
        errs["o_vs_unshifted"] = C.row_err(o, o0.double()).max().item()
        errs["dlse"] = ((got["lse"].double() - got0["lse"].double()) - (ref["lse"] - ref0["lse"])).abs().max().item()
        if errs["o_vs_unshifted"] > tol_o:
            fails.append("o_vs_unshifted")
        if errs["dlse"] > tol_lse:
            fails.append("dlse")
    print("COND %s %s %+d %s" % (path.name, profile, shift, " ".join("%s=%.3e" % kv for kv in errs.items())))
    assert not fails, (fails, errs, path.tol)


def _keep_bits(keep, B, Lq, Lk):
    """flash.hip's keep bitmap -> bool [B, 1, Lq, Lk]: bit (k & 31) of word [(bh * Lq + q) * kw + k / 32],
    kw = 2 * ceil(Lk / 64)"""
    kw = 2 * (-(-Lk // 64))
    words = keep.cpu().view(B, Lq, kw).to(torch.int64) & 0xFFFFFFFF
    kk = torch.arange(Lk)
    return ((words[:, :, kk // 32] >> (kk % 32)) & 1).bool().view(B, 1, Lq, Lk)


@pytest.mark.parametrize("profile,shift", [(p, 0.0) for p in C.PROFILES] + [("ramp", 60.0), ("saw", -60.0)])
@pytest.mark.parametrize("path", _vfold_paths(), ids=repr)
def test_vfold_dropout_row_sums_on_structured_scores(path, profile, shift):
    """p_drop = 0.1 with the keep bitmap: u' = [(P o keep / 0.9) mem | its row sum | 0] against float64 on the
    kernel's own keep bits -- the one case in which rd[u] * alpha rescales a nonzero dropped-probability sum"""
    ops = _ops()
    tol_o, tol_lse, _ = path.tol
    q, k, mem, _, _ = _ref(path, profile, shift)
    B, _, Lq, Lk, D = path.shape
    p_drop = 0.1
    u = torch.full((B, Lq, 1, 72), float("nan"), device=DEV, dtype=torch.bfloat16)
    lse = torch.full((B, 1, Lq), float("nan"), device=DEV)
    keep = torch.zeros(ops.keep_words(B, 1, Lq, Lk), device=DEV, dtype=torch.int32)
    with _knobs(**path.knobs):
        _check_plan(path)
        ops.attn_fwd_vfold(q.to(DEV), k.to(DEV), mem.to(DEV), u, lse, D ** -0.5, p_drop, 11, idx0=6, keep=keep)
        torch.cuda.synchronize()
    u, lse = u.cpu(), lse.cpu()
    assert torch.isfinite(u.float()).all() and torch.isfinite(lse).all()
    bits = _keep_bits(keep, B, Lq, Lk)
    assert 0.85 < bits.double().mean().item() < 0.95
    ref = C.reference(q, k, mem, D ** -0.5, keep=bits, p_drop=p_drop)
    # a gain-11 row whose spike key is dropped keeps only probabilities below 2^-149: exactly 0 in fp32, so
    # rows below fp32's range are compared absolutely
    eo = C.row_err(u[..., :64], ref["o"], floor=2.0 ** -120).max().item()
    rs = ref["rowsum"].transpose(1, 2)  # [B, Lq, 1]
    er = ((u[..., 64].double() - rs).abs() / rs.clamp_min(1.0)).max().item()
    el = (lse.double() - ref["lse"]).abs().max().item()
    print("COND %s-drop %s %+d o=%.3e rowsum=%.3e lse=%.3e" % (path.name, profile, shift, eo, er, el))
    assert torch.all(u[..., 65:] == 0)
    assert eo <= tol_o and er <= tol_o and el <= tol_lse, (eo, er, el)
    if profile in ("ramp", "saw"):  # the row sums do differ from 1: the check above is not vacuous
        assert (rs - 1).abs().max().item() > 0.05


def _cpu_windows(x, fill, ws):
    """[B, H, W, C] -> [B * nW, ws * ws, C] in the window order of ops.window_pad, padded positions = fill [C]"""
    B, H, W, Cc = x.shape
    Hp, Wp = -(-H // ws) * ws, -(-W // ws) * ws
    xp = fill.to(x.dtype).expand(B, Hp, Wp, Cc).clone()
    xp[:, :H, :W] = x
    return xp.view(B, Hp // ws, ws, Wp // ws, ws, Cc).permute(0, 1, 3, 2, 4, 5).reshape(-1, ws * ws, Cc)


def test_padded_window_mode_on_structured_scores():
    """the padded-window flash mode (s2h_flash_win_fwd / _bwd) and the partitioned launches it must equal bit
    for bit, with a rank-one component on the q and k thirds of qkv and a bias row whose key outscores every
    real key for the high-gain queries (a padded key wins the softmax), against float64 over the windows"""
    from test_hiera_win_map_gpu import _mapped, _partitioned, _real_mask
    ops = _ops()
    ops.wgrad_workspace(DEV)
    B, H, W, nh, hd, ws = 32, 16, 16, 2, 56, 14
    d, L, scale = nh * hd, ws * ws, hd ** -0.5
    t = torch.arange(B * H * W)
    gq = torch.tensor(C.GAINS, dtype=torch.float64)[t % 8]
    gk = 6.3 * (t % (H * W)).double() / (H * W - 1)  # a ramp in token order: the full window rescales
    gen = torch.Generator().manual_seed(23)
    qkv = torch.empty(B, H, W, 3, nh, hd, dtype=torch.float64)
    qkv[:, :, :, 0] = C.structured_rows(gq, nh, hd, 5, 0).view(B, H, W, nh, hd)
    qkv[:, :, :, 1] = C.structured_rows(gk, nh, hd, 5, 1).view(B, H, W, nh, hd)
    qkv[:, :, :, 2] = torch.randn(B, H, W, nh, hd, generator=gen, dtype=torch.float64)
    bias = 0.5 * torch.randn(3, nh, hd, generator=gen, dtype=torch.float64)
    bias[1] = C.structured_rows([8.0], nh, hd, 5, 2)[0]  # 8 > 6.3: the padded key is the row maximum
    qkv = qkv.view(B, H, W, 3 * d).to(DEV, torch.bfloat16)
    bias = bias.view(3 * d).bfloat16().float().to(DEV)
    do = torch.randn(B, H, W, d, generator=gen).to(DEV, torch.bfloat16)
    gb0 = torch.zeros(3 * d, device=DEV)
    o0, lse0, dqkv0, gb_ref = _partitioned(qkv, bias, do, gb0, ws, nh)
    o1, lse1, dqkv1, gb_new, _ = _mapped(qkv, bias, do, gb0, ws, nh)
    torch.cuda.synchronize()
    real = _real_mask(B, H, W, ws, nh)  # [B * nW, nh, L]
    assert torch.equal(o1, o0) and torch.equal(dqkv1, dqkv0) and torch.equal(gb_new, gb_ref)
    assert torch.equal(lse1.view(lse0.shape)[real], lse0[real])
    # float64 over the partitioned windows
    win = _cpu_windows(qkv.cpu().double(), bias.cpu().double(), ws).view(-1, L, 3, nh, hd)
    dow = _cpu_windows(do.cpu().double(), torch.zeros(d, dtype=torch.float64), ws).view(-1, L, nh, hd)
    ref = C.reference(win[:, :, 0], win[:, :, 1], win[:, :, 2], scale, do=dow)
    realc = real.cpu()
    rq = realc.transpose(1, 2)  # [nwin, L, nh]
    # the inputs do what they claim: in the windows with padding the high-gain queries' best key is padded,
    # and the full windows' ramp rescales
    best = ref["s"].argmax(-1)                                      # [nwin, nh, L]
    padded_best = ~torch.gather(realc, 2, best)
    hi = (_cpu_windows(gq.view(B, H, W, 1), torch.zeros(1, dtype=torch.float64), ws) >= 2.5)[..., 0]  # [nwin, L]
    partial = ~realc.all(-1).all(-1)                                # [nwin]
    sel = (hi[:, None, :] & realc)[partial]
    assert sel.any() and padded_best[partial][sel].all()
    count, _ = C.regime(ref["s"][~partial] * C.LOG2E)
    assert (count > 0).any()
    tol_o, tol_lse, tol_g = TOL_FLASH
    ow = _cpu_windows(o1.cpu().double(), torch.zeros(d, dtype=torch.float64), ws).view(-1, L, nh, hd)
    eo = C.row_err(ow, ref["o"])[rq].max().item()
    el = (lse1.cpu().double().view(-1, nh, L) - ref["lse"])[realc].abs().max().item()
    gw = _cpu_windows(dqkv1.cpu().double(), torch.zeros(3 * d, dtype=torch.float64), ws).view(-1, L, 3, nh, hd)
    eg = {n: C.tensor_err(gw[:, :, i][rq], ref[n][rq]) for i, n in enumerate(("dq", "dk", "dv"))}
    print("COND flash-winmap structured +0 o=%.3e lse=%.3e %s" % (eo, el, " ".join("%s=%.3e" % kv for kv in eg.items())))
    assert eo <= tol_o and el <= tol_lse and all(e <= tol_g for e in eg.values()), (eo, el, eg)
