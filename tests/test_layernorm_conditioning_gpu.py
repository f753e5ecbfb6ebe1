"""Every HIP LayerNorm of the step on the rows of ln_cases.py -- a large offset (300 +- 0.5, 30 +- 0.05, both
signs), two outlier channels, constant rows, a constant row with one channel one bf16 ulp up, variance far
below eps, variance 1e8, zeros, and randn -- at eps 1e-6 and 1e-5, against the float64 models there, per row
(per column for dgamma / dbeta), never against another kernel path and never scaled by a tensor maximum:

  ops.layernorm_fwd / layernorm_bwd   every <G, K> that norm.hip plan() selects (each case recomputes the rule
      from C, the strides and the addresses it really passes, and asserts the path it names), the scalar
      kernels at C 20 / 37 and at C 256 with the base one element off; forward also from a strided source
      (row stride C + 8: vector, C + 1: scalar) and with the fused pre-add (per row and broadcast, the sum
      really rounding in bf16 on the offset rows, xsum bit-exact); backward from the forward's own saved
      mean / rstd, with dres, with accumulate, into non-zero dgamma / dbeta, and 4099 rows at C 512 (the
      block count capped at 1024, a ragged last pass of the grid-stride loop);
  s2h_layernorm_fwd_pe                y against float64, ype the exact fp32 sum of the stored y and the table;
  ops.linear_add_ln                   LayerNorm of the kernel's own residual stream xs (regime rows + a small
      projection, so the sum rounds in bf16);
  ops.linear_dgrad_ln_bwd             LN'(dy @ w) with float64 statistics;
  s2h_convt2_ln_gelu                  LayerNorm and erf-GELU of the kernel's own `pre`;
  ops.mask_down_stage                 w = 0 and bias = the row: gelu(LN2d(row)) at every output pixel; and a
      small non-zero w.

The tolerances are ln_cases.py's, fixed from the fp32 model on the CPU; test_layernorm_conditioning_host.py
proves that each assertion can fail by more than 10x.

ops.layernorm_bwd passes ldx = lddy = lddx = C: a strided backward is unreachable from Python, so only the
forward is run from strided rows.  dt_layernorm (csrc/decoder_tok.hip) forms its input inside the launch: it
is pinned on the same regimes by dec_tok_cases.py and test_decoder_tok_kernels_gpu.py.

Observed maxima on an MI355X over all cases, as error / tolerance (the module prints them at teardown, -s).
Where the output is bf16, y / dx / the GELU sit at 0.97 .. 0.99: the store's own rounding uses up to the
whole of its half-ulp term, as it does for the fp32 model; the fp32 outputs and mean / rstd show the
arithmetic.  The clean fp32 model's maxima (ln_cases.py) are mean 0.19, rstd 0.20, y 0.19, dx 0.24.
  norm.hip vector  fp32   mean 0.19   rstd 0.15  y 0.14   dx 0.16   dgamma 0.034   dbeta 0.071
  norm.hip vector  bf16   mean 0.0062 rstd 0.18  y 0.99   dx 0.99   dgamma 0.0017  dbeta 0.018
  norm.hip scalar  fp32   mean 0.14   rstd 0.15  y 0.16   dx 0.14   dgamma 0.0031  dbeta 0.036
  norm.hip scalar  bf16   mean 0.018  rstd 0.15  y 0.99   dx 0.97   dgamma 0.0002  dbeta 0.018
  layernorm_fwd_pe        mean 0.0001 rstd 0.13  y 0.99   (ype exact)
  linear_add_ln           mean 0.0004 rstd 0.14  y 0.98
  linear_dgrad_ln_bwd     dx 0.97   dgamma 2e-5   dbeta 0.0017
  convt2_ln_gelu          mean 2e-5   rstd 0.12  y 0.97   post 0.85
  mask_down_stage  fp32   gelu(LN2d) 0.28, with small w 0.013;  bf16 0.93 / 0.88
Every exact assertion (xsum, ype, the path taken, the refusals) held; nothing is above its tolerance, and
mean / rstd are nowhere above a fifth of theirs.  No kernel was changed.

On a build whose vector forward takes the variance as E[x^2] - mu^2 (tried once, not kept) 13 cases here
fail -- every fp32 size, bf16 from C = 112 up, the 4099-row case, layernorm_fwd_pe at C = 512 -- while all
20 cases of test_kernels_gpu.py::test_layernorm pass it.  bf16 rows of C <= 64 pass it too: with fused
multiply-adds the squares of bf16 values and their short sums are exact in fp32, so there the one-pass
form is not wrong.
"""
import math

import numpy as np
import pytest
import torch

import ln_cases as L

pytestmark = pytest.mark.gpu
DEV = "cuda"
INVALID = 1  # hipErrorInvalidValue
MAXIMA = {}


def _ops():
    from sam2_video.kernels import ops
    return ops


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    for k in sorted(MAXIMA):
        print(f"ln maxima {k[0]:>16} {k[1]:>9}: {MAXIMA[k][0]:.3g} at {MAXIMA[k][1]}")
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _tt(dtype):
    return torch.bfloat16 if dtype == "bf16" else torch.float32


def dev(a, dtype="fp32"):
    """numpy fp32 holding values of `dtype` -> device tensor of that type (exact)"""
    return torch.tensor(np.asarray(a, dtype=np.float32), device=DEV).to(_tt(dtype))


def host(t):
    return t.detach().float().cpu().numpy()


def misaligned(t):
    """the same values, contiguous, with the base one element past a 16-byte boundary"""
    buf = torch.empty(t.numel() + 16, dtype=t.dtype, device=DEV)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 != 0
    return v


def hold(family, res, names, case):
    """every assertion of a check <= 1; the maxima kept for the module's report"""
    for k, r in res.items():
        v, where = L.worst(r, names if len(r) == len(names) else None)
        if v > MAXIMA.get((family, k), (-1, ""))[0]:
            MAXIMA[(family, k)] = (v, f"{where} {case}")
    for k, r in res.items():
        v, where = L.worst(r, names if len(r) == len(names) else None)
        assert v <= 1.0, f"{family} {case}: {k} is {v:.3g} x its tolerance at {where}"


def fwd_path(C, dtype, x, y, add=None, bcast=False, xsum=None):
    """norm.hip ln_fwd's plan() from what ops.layernorm_fwd passes"""
    ldb = 0 if (add is None or bcast) else add.stride(0)
    return L.plan(C, dtype, (x.stride(0), ldb, C),
                  (x.data_ptr(), 0 if add is None else add.data_ptr(), 0 if xsum is None else xsum.data_ptr(),
                   y.data_ptr()))


def bwd_path(C, dtype, x, dy, dx, dres=None):
    return L.plan(C, dtype, (C, C, C, C if dres is not None else 0),
                  (x.data_ptr(), dy.data_ptr(), dx.data_ptr(), 0 if dres is None else dres.data_ptr()))


def run_fwd(family, want, dtype, C, eps, x, names, add=None, bcast=False, case=""):
    """ops.layernorm_fwd on device rows x (any stride / base) -> checks y, mean, rstd (and xsum bit-exact);
    returns (the normalised rows as numpy, mean, rstd)"""
    ops = _ops()
    gamma, beta = L.make_params(C)
    y = torch.full((x.shape[0], C), float("nan"), dtype=x.dtype, device=DEV)
    xsum = torch.full((x.shape[0], C), float("nan"), dtype=x.dtype, device=DEV) if add is not None else None
    assert fwd_path(C, dtype, x, y, add, bcast, xsum) == want, "the case does not take the path it names"
    _, mean, rstd = ops.layernorm_fwd(x, dev(gamma), dev(beta), eps, y=y, add=add, add_bcast=bcast, xsum=xsum)
    xin = host(x)
    if add is not None:
        xin = L.preadd(xin, host(add), dtype)
        assert np.array_equal(host(xsum), xin), f"{family} {case}: xsum is not round(a + b)"
    hold(f"{family} {dtype}", L.check_fwd(xin, gamma, beta, eps, host(y), host(mean), host(rstd), out=dtype), names,
         case)
    return xin, mean, rstd


def run_bwd(family, want, dtype, C, eps, x, names, mean, rstd, mode, case=""):
    """ops.layernorm_bwd from the forward's saved statistics; mode: plain / dres / accumulate"""
    ops = _ops()
    n = x.shape[0]
    gamma, _ = L.make_params(C)
    dy_h = L.make_noise(n, C, dtype, 1)
    add_h = None if mode == "plain" else L.make_noise(n, C, dtype, 2)
    dg0, db0 = (np.zeros((2, C), np.float32) if mode == "plain" else L.make_noise(2, C, "fp32", 3))
    dy = dev(dy_h, dtype)
    dres = dev(add_h, dtype) if mode == "dres" else None
    dx = dev(add_h, dtype) if mode == "accumulate" else torch.full((n, C), float("nan"), dtype=x.dtype, device=DEV)
    dg, db = dev(dg0), dev(db0)
    assert bwd_path(C, dtype, x, dy, dx, dres) == want, "the case does not take the path it names"
    ops.layernorm_bwd(x, dy, dev(gamma), mean, rstd, dx=dx, accumulate=mode == "accumulate", dgamma=dg, dbeta=db,
                      dres=dres)
    res = L.check_bwd(host(x), dy_h, gamma, eps, host(dx), host(dg), host(db), addend=add_h, dg0=dg0, db0=db0,
                      out=dtype)
    hold(f"{family} {dtype}", res, names, f"{case} bwd-{mode}")


# ------------------------------------------------------------------ 1. norm.hip, every dispatch
VEC_CASES = [("bf16", 8, 1, 1), ("bf16", 16, 2, 1), ("bf16", 32, 4, 1), ("bf16", 64, 8, 1), ("bf16", 112, 16, 1), ("bf16", 256, 32, 1),
             ("bf16", 512, 64, 1), ("bf16", 896, 64, 2), ("bf16", 1280, 64, 3), ("fp32", 4, 1, 1),
             ("fp32", 112, 32, 1), ("fp32", 256, 64, 1), ("fp32", 448, 64, 2), ("fp32", 896, 64, 5),
             ("fp32", 1280, 64, 5)]


@pytest.mark.parametrize("dtype,C,G,K", VEC_CASES, ids=[f"{d}-{C}-G{G}-K{K}" for d, C, G, K in VEC_CASES])
def test_vector_kernels(dtype, C, G, K):
    want = ("vec", G, K)
    scalar = ("scalar", 64, 1)
    xh, names = L.make_rows(C, dtype)
    x = dev(xh, dtype)
    for eps in L.EPS:
        case = f"{dtype} C={C} <{G},{K}> eps={eps}"
        _, mean, rstd = run_fwd("ln_vec", want, dtype, C, eps, x, names, case=case)
        for mode in ("plain", "dres", "accumulate"):
            run_bwd("ln_vec", want, dtype, C, eps, x, names, mean, rstd, mode, case=case)
        add = dev(L.rounding_addend(xh, dtype), dtype)
        run_fwd("ln_vec", want, dtype, C, eps, x, names, add=add, case=case + " add")
        addb = dev(L.rounding_addend(xh, dtype, True), dtype)
        run_fwd("ln_vec", want, dtype, C, eps, x, names, add=addb, bcast=True, case=case + " add_bcast")
    # strided sources: the padding holds NaN, which the statistics would show
    for pad, path in ((8, want), (1, scalar)):
        wide = torch.full((L.NROWS, C + pad), float("nan"), dtype=_tt(dtype), device=DEV)
        wide[:, :C] = x
        run_fwd("ln_vec" if path == want else "ln_scalar", path, dtype, C, 1e-6, wide[:, :C], names,
                case=f"{dtype} C={C} row stride C+{pad}")


SCALAR_CASES = [("bf16", 20, False), ("bf16", 37, False), ("fp32", 37, False), ("bf16", 256, True),
                ("fp32", 256, True)]


@pytest.mark.parametrize("dtype,C,off", SCALAR_CASES, ids=[f"{d}-{C}{'-base+1' if o else ''}" for d, C, o in SCALAR_CASES])
def test_scalar_kernels(dtype, C, off):
    """C no multiple of the vector width, and C = 256 from a base one element off: judged against float64
    on their own (the aligned C = 256 is in test_vector_kernels, against float64 too)"""
    want = ("scalar", 64, 1)
    xh, names = L.make_rows(C, dtype)
    x = dev(xh, dtype)
    if off:
        assert L.plan(C, dtype, (C, 0, C), (x.data_ptr(),))[0] == "vec"
        x = misaligned(x)
    for eps in L.EPS:
        case = f"{dtype} C={C} scalar{' base+1' if off else ''} eps={eps}"
        _, mean, rstd = run_fwd("ln_scalar", want, dtype, C, eps, x, names, case=case)
        for mode in ("plain", "dres", "accumulate"):
            run_bwd("ln_scalar", want, dtype, C, eps, x, names, mean, rstd, mode, case=case)
        add = dev(L.rounding_addend(xh, dtype), dtype)
        run_fwd("ln_scalar", want, dtype, C, eps, x, names, add=add, case=case + " add")
        addb = dev(L.rounding_addend(xh, dtype, True), dtype)
        run_fwd("ln_scalar", want, dtype, C, eps, x, names, add=addb, bcast=True, case=case + " add_bcast")


def test_backward_grid_stride_ragged_last_pass():
    """4099 rows at C = 512 bf16 (<64, 1>: 4 rows per block): 1025 blocks wanted, 1024 launched, so the
    loop's second pass holds 3 rows"""
    dtype, C, n = "bf16", 512, 4099
    assert math.ceil(n / 4) > 1024 and n - 1024 * 4 == 3
    xh, names = L.make_rows(C, dtype, n)
    x = dev(xh, dtype)
    _, mean, rstd = run_fwd("ln_vec", ("vec", 64, 1), dtype, C, 1e-6, x, names, case="4099 rows")
    run_bwd("ln_vec", ("vec", 64, 1), dtype, C, 1e-6, x, names, mean, rstd, "dres", case="4099 rows")


# ------------------------------------------------------------------ 2. LayerNorm + positional table
@pytest.mark.parametrize("C,G", [(64, 8), (128, 16), (256, 32), (512, 64)])
def test_layernorm_fwd_pe(C, G):
    from sam2_video.kernels._lib import call
    ops = _ops()
    dtype, pe_rows = "bf16", 9
    xh, names = L.make_rows(C, dtype)
    gamma, beta = L.make_params(C)
    peh = L.make_noise(pe_rows, C, dtype, 4)
    x, pe = dev(xh, dtype), dev(peh, dtype)
    for eps in L.EPS:
        y = torch.full_like(x, float("nan"))
        ype = torch.full_like(x, float("nan"))
        mean, rstd = torch.empty(L.NROWS, device=DEV), torch.empty(L.NROWS, device=DEV)
        assert L.plan(C, dtype, (C, 0, C), (x.data_ptr(), 0, 0, y.data_ptr())) == ("vec", G, 1)
        g, b = dev(gamma), dev(beta)
        call("s2h_layernorm_fwd_pe", ops.BF16, L.NROWS, C, x.data_ptr(), g.data_ptr(), b.data_ptr(), eps, y.data_ptr(),
             mean.data_ptr(), rstd.data_ptr(), pe.data_ptr(), pe_rows, ype.data_ptr(), ops.stream())
        case = f"C={C} <{G},1> eps={eps}"
        hold("ln_pe", L.check_fwd(xh, gamma, beta, eps, host(y), host(mean), host(rstd), out=dtype), names, case)
        assert np.array_equal(host(ype), L.pe_out(host(y), peh, dtype)), f"{case}: ype is not round(y + pe[row % 9])"


# ------------------------------------------------------------------ 3. GEMM epilogue LayerNorm
@pytest.mark.parametrize("N", [128, 256])
@pytest.mark.parametrize("K", [72, 256])
@pytest.mark.parametrize("p_drop", [0.0, 0.1])
def test_linear_add_ln(N, K, p_drop):
    ops = _ops()
    M = L.NROWS
    rh, names = L.make_rows(N, "bf16")
    gamma, beta = L.make_params(N)
    xh = L.make_noise(M, K, "bf16", 5)
    wh = L.make_noise(N, K, "bf16", 6, scale=1e-2)
    bh = L.make_noise(1, N, "fp32", 7, scale=0.1)[0]
    lin = xh.astype(np.float64) @ wh.astype(np.float64).T + bh
    for eps in L.EPS:
        ops.rng_offset(DEV).fill_(7)
        y, xs, mean, rstd = ops.linear_add_ln(dev(xh, "bf16"), dev(wh, "bf16"), dev(bh), dev(rh, "bf16"), dev(gamma),
                                              dev(beta), eps, drop_p=p_drop, seed=99, drop_idx0=12)
        xsh = host(xs)
        off = [i for i, n in enumerate(names) if n in ("offset300", "neg_offset")]
        assert (xsh[off].astype(np.float64) != (rh[off] + lin[off])).mean() > 0.9, "the sum must round in bf16"
        if p_drop == 0:  # the rows are still the regimes: x' = round(residual + projection)
            ref = rh + lin
            assert np.all(np.abs(xsh - ref) <= 2.0 ** -8 * np.abs(ref) + 1e-4 * np.abs(lin) + 1e-30)
        case = f"N={N} K={K} p={p_drop} eps={eps}"
        hold("linear_add_ln", L.check_fwd(xsh, gamma, beta, eps, host(y), host(mean), host(rstd), out="bf16"), names,
             case)


# ------------------------------------------------------------------ 4. dgrad GEMM + LayerNorm backward
@pytest.mark.parametrize("C", [128, 256])
@pytest.mark.parametrize("res,wgrad", [(True, True), (False, True), (True, False), (False, False)])
def test_linear_dgrad_ln_bwd(C, res, wgrad):
    ops = _ops()
    M, K = L.NROWS, 64
    xh, names = L.make_rows(C, "bf16")
    gamma, beta = L.make_params(C)
    dyh = L.make_noise(M, K, "bf16", 8)
    wh = L.make_noise(K, C, "bf16", 9, scale=C ** -0.5)
    dres_h = L.make_noise(M, C, "bf16", 2) if res else None
    dg0, db0 = L.make_noise(2, C, "fp32", 3)
    dt = dyh.astype(np.float64) @ wh.astype(np.float64)
    # the kernel's dy @ w: exact bf16 products added in fp32, at most K additions deep
    dt_err = K * L.U * (np.abs(dyh).astype(np.float64) @ np.abs(wh).astype(np.float64))
    x = dev(xh, "bf16")
    assert ops.linear_dgrad_ln_bwd_ok(dev(dyh, "bf16"), dev(wh, "bf16"), x)
    for eps in L.EPS:
        _, mean, rstd = ops.layernorm_fwd(x, dev(gamma), dev(beta), eps)
        dg, db = (dev(dg0), dev(db0)) if wgrad else (None, None)
        dx = ops.linear_dgrad_ln_bwd(dev(dyh, "bf16"), dev(wh, "bf16"), x, dev(gamma), mean, rstd,
                                     dres=dev(dres_h, "bf16") if res else None, dgamma=dg, dbeta=db)
        r = L.check_bwd(xh, dt, gamma, eps, host(dx), host(dg) if wgrad else None, host(db) if wgrad else None,
                        addend=dres_h, dg0=dg0 if wgrad else None, db0=db0 if wgrad else None, out="bf16", dy_err=dt_err)
        hold("dgrad_ln_bwd", r, names, f"C={C} dres={res} wgrad={wgrad} eps={eps}")


# ------------------------------------------------------------------ 5. transposed conv + LayerNorm2d + GELU
def test_convt2_ln_gelu():
    from sam2_video.kernels._lib import call
    ops = _ops()
    B, H, W, Co = 1, 5, 5, 64
    rows = B * 4 * H * W
    addh, names = L.make_rows(Co, "bf16", rows)
    gamma, beta = L.make_params(Co)
    Y = dev(L.make_noise(B * H * W, 4 * Co, "bf16", 10, scale=1e-2), "bf16")
    bias = dev(L.make_noise(1, Co, "fp32", 11, scale=1e-2)[0])
    add = dev(addh, "bf16").view(1, 2 * H, 2 * W, Co)
    g, b = dev(gamma), dev(beta)
    for eps in L.EPS:
        pre, y, post = (torch.full((rows, Co), float("nan"), dtype=torch.bfloat16, device=DEV) for _ in range(3))
        mean, rstd = torch.empty(rows, device=DEV), torch.empty(rows, device=DEV)
        call("s2h_convt2_ln_gelu", ops.BF16, B, H, W, Co, Y.data_ptr(), bias.data_ptr(), add.data_ptr(), 1,
             g.data_ptr(), b.data_ptr(), eps, pre.data_ptr(), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
             post.data_ptr(), ops.stream())
        ph = host(pre)
        # pre is still the regime rows (Y and the bias are ~1e-2): within their size plus a bf16 rounding
        assert np.all(np.abs(ph - addh) <= 0.1 + 2.0 ** -8 * np.abs(addh))
        case = f"convt2 eps={eps}"
        hold("convt2_ln_gelu", L.check_fwd(ph, gamma, beta, eps, host(y), host(mean), host(rstd), out="bf16"), names,
             case)
        hold("convt2_ln_gelu", {"post": L.check_gelu_of_ln(ph, gamma, beta, eps, host(post), "bf16", y_out="bf16")},
             names, case)


# ------------------------------------------------------------------ 6. mask downsampler stage
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("cout,cin", [(4, 1), (16, 4), (64, 16)])
def test_mask_down_stage_layernorm2d(dtype, cout, cin):
    """w = 0, bias = the row: every output pixel's pre-norm vector is that row, exactly"""
    ops = _ops()
    rh, names = L.make_rows(cout, "fp32", len(L.REGIMES))
    gamma, beta = L.make_params(cout)
    x = dev(L.make_noise(9, cin, dtype, 12).reshape(1, 3, 3, cin), dtype)
    w = torch.zeros(cout, cin, 3, 3, device=DEV)
    for eps in L.EPS:
        got = np.stack([host(ops.mask_down_stage(x, w, dev(rh[i]), dev(gamma), dev(beta), eps)).reshape(4, cout)
                        for i in range(len(names))])  # [regime, pixel, cout]
        for p in range(4):
            r = L.check_gelu_of_ln(rh, gamma, beta, eps, got[:, p], dtype)
            hold(f"mask_down {dtype}", {"gelu_ln": r}, names, f"cout={cout} eps={eps} pixel {p}")


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_mask_down_stage_small_weights(dtype):
    """a small non-zero w on top of bias = the row: the pre-norm vector is bias + conv, formed in fp32 over
    9 cin + 1 additions of values of the row's size (x_err)"""
    ops = _ops()
    cout, cin = 64, 16
    rh, names = L.make_rows(cout, "fp32", len(L.REGIMES))
    gamma, beta = L.make_params(cout)
    xh = L.make_noise(9, cin, dtype, 12).reshape(1, 3, 3, cin)
    wh = L.make_noise(cout * cin, 9, "fp32", 13, scale=1e-3).reshape(cout, cin, 3, 3)
    conv = torch.nn.functional.conv2d(torch.tensor(xh, dtype=torch.float64).permute(0, 3, 1, 2),
                                      torch.tensor(wh, dtype=torch.float64), stride=2, padding=1)
    conv = conv.permute(0, 2, 3, 1).reshape(4, cout).numpy()
    for eps in L.EPS:
        got = np.stack([host(ops.mask_down_stage(dev(xh, dtype), dev(wh), dev(rh[i]), dev(gamma), dev(beta), eps))
                        .reshape(4, cout) for i in range(len(names))])
        for p in range(4):
            pre = rh.astype(np.float64) + conv[p]
            x_err = (9 * cin + 1) * L.U * np.abs(pre).max(axis=1)
            r = L.check_gelu_of_ln(pre, gamma, beta, eps, got[:, p], dtype, x_err=x_err)
            hold(f"mask_down {dtype}", {"gelu_ln_w": r}, names, f"small w eps={eps} pixel {p}")


# ------------------------------------------------------------------ ABI
def test_abi_refusals():
    """C = 0 and C = 1281 are refused with hipErrorInvalidValue, rows = 0 succeeds without a launch (the
    buffers are large enough for every shape named, launched or not)"""
    from sam2_video.kernels._lib import lib
    ops = _ops()
    h = lib()
    for tt, code in ((torch.bfloat16, ops.BF16), (torch.float32, ops.F32)):
        x = torch.zeros(4, 1288, dtype=tt, device=DEV)
        y, dy, dx = torch.zeros_like(x), torch.zeros_like(x), torch.zeros_like(x)
        g, b = torch.ones(1288, device=DEV), torch.zeros(1288, device=DEV)
        mean, rstd = torch.zeros(4, device=DEV), torch.ones(4, device=DEV)
        for rows, C, rc in ((4, 1281, INVALID), (4, 0, INVALID), (0, 256, 0), (0, 1281, 0)):
            ld = max(C, 1)
            assert h.s2h_layernorm_fwd(code, rows, C, x.data_ptr(), ld, None, ld, 0, None, g.data_ptr(), b.data_ptr(),
                                       1e-6, y.data_ptr(), ld, mean.data_ptr(), rstd.data_ptr(), ops.stream()) == rc
            assert h.s2h_layernorm_bwd(code, rows, C, x.data_ptr(), ld, dy.data_ptr(), ld, g.data_ptr(),
                                       mean.data_ptr(), rstd.data_ptr(), dx.data_ptr(), ld, 0, None, ld, None, None,
                                       None, ops.stream()) == rc
            if tt == torch.bfloat16:
                assert h.s2h_layernorm_fwd_pe(code, rows, C, x.data_ptr(), g.data_ptr(), b.data_ptr(), 1e-6,
                                              y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), dy.data_ptr(), 1,
                                              dx.data_ptr(), ops.stream()) == rc
        torch.cuda.synchronize()
        assert float(y.abs().max()) == 0 and float(dx.abs().max()) == 0  # nothing ran
