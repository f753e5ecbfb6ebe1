"""Shared by test_layernorm_conditioning_host.py and test_layernorm_conditioning_gpu.py: the row LayerNorm
of csrc/norm.hip (vector and scalar kernels), csrc/gemm_epi.h (epilogue8_ln and the fused backward),
csrc/elementwise.hip (convt2_ln_gelu) and csrc/memenc.hip (the LayerNorm2d of mask_down_stage) on rows that
are not randn: a large offset (300 +- 0.5, 30 +- 0.05), two outlier channels, constant rows, a constant row
with one channel one bf16 ulp up, variance far below eps, variance 1e8, zeros.  There mean / std is 10 .. 1e3
and rstd reaches 1 / sqrt(eps), so a one-pass variance, a misplaced eps or statistics taken before the bf16
rounding of a fused sum are off by 1e3 .. 1e4 times the two-pass fp32 error; on randn rows they are not.

Everything is numpy.  make_rows() gives 70 rows (7 of each regime, ragged against every rows-per-block of
the kernels), already rounded to the storage type, so the float64 models see what the kernels read.

Models: fwd64 / bwd64 / preadd / pe_out are the reference (float64; preadd and pe_out are the two places
where the kernels' result is defined by an fp32 sum rounded to the storage type, and are exact).  fwd32 /
bwd32 are an fp32 model of the kernels' own arithmetic -- G lanes per row, each summing its K chunks of VEC
values in order, then a xor butterfly; mu = s / C, q = sum (x - mu)^2, rs = 1 / sqrt(q / C + eps) -- with
switchable DEFECTS.  The host file proves that the clean model holds every assertion with a factor 4 to
spare and that each defect breaks a named one by more than 10x; the GPU file runs the same checks on the HIP
kernels.  The tolerance constants below were set from the clean fp32 model alone, never from the kernels.

A check returns {assertion: error / tolerance, one figure per row (per column for dgamma / dbeta)}; nothing
is scaled by a whole-tensor maximum.  With u = 2^-24 and D = depth(C) = min(C, 64), the longest chain of
additions any of the kernels uses (so D u max|x_r| bounds the error of the fp32 mean; at C <= 64 it is the
C u max|x| of a plain sum), per row r and element e, against float64:

  mean   u |mean| + C_MEAN u D max|x_r|
  rstd   relative, C_RSTD (8 u + (rstd_r u D max|x_r|)^2)   (sum (x - mu')^2 = sum (x - mu)^2 + C dmu^2:
                                                             the mean's error enters in second order)
  y      rnd(y) + 4 u (|gamma xhat| + |beta|) + C_Y |gamma_e| rstd_r u D max|x_r|
  dx     rnd(dx) + 4 u (|rs g| + |rs s1| + |rs xhat s2| + |addend|)
         + C_DX rstd_r max|g_r| (1 + |xhat_re|) (1 + max|xhat_r|) u D (1 + rstd_r max|x_r|)
         (s1, s2 are fp32 sums of depth D; xhat carries the saved mean's error, rstd_r u D max|x_r|)
  dgamma ulp + C_DG (sqrt(rows) u sum_r |dy xhat| + sum_r |dy| rstd_r u D max|x_r|)   per column
  dbeta  ulp + C_DG sqrt(rows) u sum_r |dy|                                           per column
  rnd(v) = 2^-8 |v| for bf16 outputs (half an ulp at worst), 2^-23 |v| for fp32 ones.

The constants were not fixed in advance.  Clean fp32 model against float64, maximum over all regimes, the
C of SIZES, eps 1e-6 / 1e-5, both types, the vector and the scalar lane layout, the plain forward and both
pre-adds, the backward with dres into non-zero dgamma / dbeta, as a fraction of the tolerance *without* the
output rounding (test_layernorm_conditioning_host.py::test_clean_model_within_quarter prints them with -s):
  mean   0.189  fp32 C 4 offset300       (C_MEAN 2; with 1 it is 0.34: four values of 300 lose ~2 u |mean|)
  rstd   0.196  bf16 C 896 outlier       (C_RSTD 2; with 1 it is 0.39)
  y      0.194  fp32 C 448 tiny          (C_Y 3; with 2 a tiny row at fp32 C 4 is at 0.244)
  dx     0.238  bf16 C 16 large          (C_DX 2; with 1 a zero row at fp32 C 4 is at 0.32)
  dgamma 0.037, dbeta 0.152              (C_DG 2; with 1 dbeta is at 0.29)
Each constant is the smallest of 1, 2, 3 that keeps its figure under a quarter with some room.  With the
output rounded to bf16 the clean model reaches 0.99 of rnd(v) by construction (a value half an ulp from a
tie), so the quarter is asserted on the fp32 value and <= 1 on the rounded one.

dt_layernorm (csrc/decoder_tok.hip) forms its input inside the launch: the same regimes and check_fwd reach it
through dec_tok_cases.py, test_decoder_tok_host.py and test_decoder_tok_kernels_gpu.py."""
import functools
import math

import numpy as np

U = 2.0 ** -24
F32, F64 = np.float32, np.float64
REGIMES = ["randn", "offset300", "offset30", "outlier", "const", "const_ulp", "tiny", "large", "zero", "neg_offset"]
NROWS = 70
CONST = 3.140625  # exact in bf16; the bf16 ulp in [2, 4) is 2^-6
BF16_ULP_AT_CONST = 2.0 ** -6
EPS = [1e-6, 1e-5]
# (dtype, C) of every plan() dispatch the GPU file runs, and the scalar sizes
SIZES = [("bf16", 8), ("bf16", 32), ("bf16", 64), ("bf16", 112), ("bf16", 256), ("bf16", 512), ("bf16", 896),
         ("bf16", 1280), ("fp32", 4), ("fp32", 112), ("fp32", 256), ("fp32", 448), ("fp32", 896), ("fp32", 1280),
         ("bf16", 20), ("bf16", 37), ("fp32", 37), ("bf16", 128), ("bf16", 16)]

C_MEAN, C_RSTD, C_Y, C_DX, C_DG = 2.0, 2.0, 3.0, 2.0, 2.0

DEFECTS = {
    "one_pass": "variance as E[x^2] - mu^2",
    "eps_outside": "rs = 1 / (sqrt(var) + eps)",
    "bessel": "variance divided by C - 1",
    "stats_before_round": "mean / rstd of a + b before it is rounded to bf16 (y from the rounded sum)",
    "padded_count": "mean / variance divided by the padded width G K VEC instead of C",
    "bwd_s2_no_gamma": "backward s2 = mean(dy xhat) instead of mean(dy gamma xhat)",
    "bwd_means_no_rstd": "backward dx = rs g - s1 - xhat s2",
    "dgamma_x": "dgamma = sum dy x instead of sum dy xhat",
    "bwd_addend_dropped": "backward ignores dres / the accumulate addend",
    "mean_dead_lane": "the last live chunk left out of the sums (a dead-lane test off by one)",
}


def f32(v):
    """the value a C float argument takes"""
    return float(F32(v))


def round_bf16(a):
    """fp32 -> bf16 (round to nearest even) -> fp32, finite values"""
    b = np.ascontiguousarray(a, dtype=F32).view(np.uint32)
    r = (b + np.uint32(0x7FFF) + ((b >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return r.view(F32)


def round_to(a, dtype):
    a = np.asarray(a, dtype=F32)
    return round_bf16(a) if dtype == "bf16" else a.copy()


# ------------------------------------------------------------------ the kernels' dispatch rule
def vec_of(dtype):
    return 8 if dtype == "bf16" else 4


def plan(C, dtype, lds=(), ptrs=()):
    """norm.hip plan(): ("vec", G, K) or ("scalar", 64, 1) from C, the row strides (elements) and the base
    addresses (bytes; 0 = absent)"""
    VEC = vec_of(dtype)
    if C % VEC or any(ld % VEC for ld in lds) or any(p and p % 16 for p in ptrs):
        return ("scalar", 64, 1)
    NC = C // VEC
    if NC <= 64:
        G = 1
        while G < NC:
            G <<= 1
        return ("vec", G, 1)
    K = (NC + 63) // 64
    if K > 5:
        return ("scalar", 64, 1)
    return ("vec", 64, 5 if K == 4 else K)


def lanes(C, dtype, scalar=False):
    """(G, K, VEC) of the lane layout that sums a row: the vector plan, or the scalar kernels' 64 lanes
    striding single elements"""
    p = plan(C, dtype)
    if scalar or p[0] == "scalar":
        return 64, (C + 63) // 64, 1
    return p[1], p[2], vec_of(dtype)


# ------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def make_rows(C, dtype, n=NROWS, seed=0):
    """(x [n, C] fp32 holding values of `dtype`, [regime name of each row]); row i is regime i % 10.
    Shared: do not write into it."""
    g = np.random.default_rng(7919 * seed + 31 * C + (dtype == "bf16"))
    x = np.zeros((n, C), dtype=F64)
    names = []
    for i in range(n):
        name = REGIMES[i % len(REGIMES)]
        names.append(name)
        z = g.standard_normal(C)
        if name == "randn":
            x[i] = z
        elif name == "offset300":
            x[i] = 300 + 0.5 * z
        elif name == "offset30":
            x[i] = 30 + 0.05 * z
        elif name == "outlier":
            x[i] = z
            x[i, 3 % C] = 400.0
            x[i, C - 2] = -250.0
        elif name == "const":
            x[i] = CONST
        elif name == "const_ulp":
            x[i] = CONST
            x[i, (5 * i + 1) % C] = CONST + BF16_ULP_AT_CONST
        elif name == "tiny":
            x[i] = 1e-4 * z
        elif name == "large":
            x[i] = 1e4 * z
        elif name == "neg_offset":
            x[i] = -(300 + 0.5 * z)
    x = round_to(x.astype(F32), dtype)
    x.setflags(write=False)
    return x, tuple(names)


@functools.lru_cache(maxsize=None)
def make_params(C, seed=0):
    """gamma (both signs, some near 0) and beta, fp32"""
    g = np.random.default_rng(104729 * seed + C)
    gamma = (1 + 0.6 * g.standard_normal(C)).astype(F32)
    beta = (0.3 * g.standard_normal(C)).astype(F32)
    gamma.setflags(write=False)
    beta.setflags(write=False)
    return gamma, beta


@functools.lru_cache(maxsize=None)
def make_noise(n, C, dtype, seed, scale=1.0):
    """randn * scale in `dtype`: dy, dres, the accumulate target, a PE table"""
    g = np.random.default_rng(15485863 * seed + 131 * C + n)
    v = round_to((scale * g.standard_normal((n, C))).astype(F32), dtype)
    v.setflags(write=False)
    return v


def rounding_addend(x, dtype, bcast=False):
    """an addend b (in `dtype`) for the fused pre-add such that a + b is inexact in `dtype` on the offset
    rows: 0.37 .. 0.63 of the spacing of x there (|x| ~ 300 in bf16 has spacing 2), per row or one
    broadcast row"""
    n, C = x.shape
    g = np.random.default_rng(C + 5 * n + bcast)
    b = 0.7 + 0.5 * g.random((1 if bcast else n, C))
    return round_to(b.astype(F32), dtype)


def preadd(a, b, dtype):
    """the residual stream the kernels store and normalise: the fp32 sum a + b rounded once to `dtype`"""
    return round_to(np.asarray(a, F32) + np.asarray(b, F32), dtype)


def pe_out(y_stored, pe, dtype):
    """s2h_layernorm_fwd_pe: ype = round_T(y as stored, in T, + pe[row % pe_rows]), an fp32 sum"""
    n = y_stored.shape[0]
    return round_to(np.asarray(y_stored, F32) + np.asarray(pe, F32)[np.arange(n) % pe.shape[0]], dtype)


# ------------------------------------------------------------------ float64 models
def fwd64(x, gamma, beta, eps):
    x = np.asarray(x, F64)
    mean = x.mean(axis=1)
    d = x - mean[:, None]
    rstd = 1.0 / np.sqrt((d * d).mean(axis=1) + f32(eps))
    xh = d * rstd[:, None]
    return xh * np.asarray(gamma, F64) + np.asarray(beta, F64), mean, rstd


def bwd64(x, dy, gamma, eps, addend=None, dg0=None, db0=None):
    """dx = rstd (g - mean g - xhat mean(g xhat)) [+ addend], g = dy gamma; dgamma = dg0 + sum_r dy xhat,
    dbeta = db0 + sum_r dy.  addend is dres, or the previous dx when accumulating."""
    x, dy, gamma = np.asarray(x, F64), np.asarray(dy, F64), np.asarray(gamma, F64)
    _, mean, rstd = fwd64(x, gamma, 0 * gamma, eps)
    xh = (x - mean[:, None]) * rstd[:, None]
    g = dy * gamma
    dx = rstd[:, None] * (g - g.mean(axis=1)[:, None] - xh * (g * xh).mean(axis=1)[:, None])
    if addend is not None:
        dx = dx + np.asarray(addend, F64)
    dg = (dy * xh).sum(axis=0) + (0 if dg0 is None else np.asarray(dg0, F64))
    db = dy.sum(axis=0) + (0 if db0 is None else np.asarray(db0, F64))
    return dx, dg, db


def gelu64(v):
    v = np.asarray(v, F64)
    return 0.5 * v * (1.0 + np.vectorize(math.erf)(v / math.sqrt(2.0)))


# ------------------------------------------------------------------ fp32 model of the kernels' arithmetic
def _lane_sum(v, G, K, VEC, drop_last=False):
    """sum over each row of v [R, C] fp32 as G lanes do: lane j adds chunks j, j + G, .. (VEC values each) in
    order, then the lanes fold by halves (the xor butterfly's order)"""
    R, C = v.shape
    w = np.zeros((R, G * K * VEC), dtype=F32)
    w[:, :C] = v
    if drop_last:
        w[:, C - VEC:C] = 0
    w = w.reshape(R, K, G, VEC)
    s = np.zeros((R, G), dtype=F32)
    for k in range(K):
        for j in range(VEC):
            s = s + w[:, k, :, j]
    while s.shape[1] > 1:
        h = s.shape[1] // 2
        s = s[:, :h] + s[:, h:]
    return s[:, 0]


def fwd32(x, gamma, beta, eps, G, K, VEC, defects=(), add=None, dtype="fp32"):
    """(y fp32 before the store's rounding, mean, rstd, xsum or None) as the kernels compute them; `add`
    [R or 1, C] is the fused pre-add"""
    x = np.asarray(x, F32)
    R, C = x.shape
    xsum, stat_src = None, x
    if add is not None:
        raw = x + np.asarray(add, F32)
        x = xsum = round_to(raw, dtype)
        stat_src = raw if "stats_before_round" in defects else x
    n = F32(G * K * VEC if "padded_count" in defects else C)
    drop = "mean_dead_lane" in defects
    mu = _lane_sum(stat_src, G, K, VEC, drop) / n
    if "one_pass" in defects:
        var = _lane_sum(stat_src * stat_src, G, K, VEC, drop) / n - mu * mu
        var = np.maximum(var, F32(0))
    else:
        d = stat_src - mu[:, None]
        var = _lane_sum(d * d, G, K, VEC, drop) / (F32(C - 1) if "bessel" in defects else n)
    e = F32(eps)
    rs = F32(1) / (np.sqrt(var) + e) if "eps_outside" in defects else F32(1) / np.sqrt(var + e)
    y = (x - mu[:, None]) * rs[:, None] * np.asarray(gamma, F32) + np.asarray(beta, F32)
    return y.astype(F32), mu.astype(F32), rs.astype(F32), xsum


def bwd32(x, dy, gamma, mean, rstd, G, K, VEC, defects=(), addend=None, dg0=None, db0=None):
    """(dx fp32 before the store's rounding, dgamma, dbeta) from the forward's saved fp32 mean / rstd"""
    x, dy, gamma = np.asarray(x, F32), np.asarray(dy, F32), np.asarray(gamma, F32)
    C = F32(x.shape[1])
    mu, rs = np.asarray(mean, F32)[:, None], np.asarray(rstd, F32)[:, None]
    xh = (x - mu) * rs
    g = dy * gamma
    s1 = (_lane_sum(g, G, K, VEC) / C)[:, None]
    s2 = (_lane_sum((dy if "bwd_s2_no_gamma" in defects else g) * xh, G, K, VEC) / C)[:, None]
    dx = rs * g - s1 - xh * s2 if "bwd_means_no_rstd" in defects else rs * (g - s1 - xh * s2)
    if addend is not None and "bwd_addend_dropped" not in defects:
        dx = dx + np.asarray(addend, F32)
    dg = np.zeros(x.shape[1], F32)
    db = np.zeros(x.shape[1], F32)
    for r in range(x.shape[0]):  # rows in order, as a block's partial sums
        dg = dg + dy[r] * (x[r] if "dgamma_x" in defects else xh[r])
        db = db + dy[r]
    if dg0 is not None:
        dg, db = dg + np.asarray(dg0, F32), db + np.asarray(db0, F32)
    return dx.astype(F32), dg, db


# ------------------------------------------------------------------ checks
MAX_DEPTH = 64


def depth(C):
    """the longest chain of fp32 additions any of the kernels uses for a sum over C channels: min(C, 64).
    mask_down_stage adds its 64 channels in order; norm.hip's lanes add K VEC <= 40 values, then 6 butterfly
    steps (the scalar kernels <= 20 + 6); convt2_ln_gelu 8 + 3; the GEMM epilogue 8 + 5.  A sum of depth d
    over values bounded by m is within d u m of the exact mean: the D of the tolerances above."""
    return min(C, MAX_DEPTH)


def _rnd(ref, dtype):
    return np.abs(ref) * (2.0 ** -8 if dtype == "bf16" else 2.0 ** -23 if dtype == "fp32" else 0.0)


def _ratio(err, tol):
    """error / tolerance; 0 where the error is 0 (a zero tolerance asks for the exact value)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(err == 0, 0.0, err / tol)


def check_fwd(x, gamma, beta, eps, y=None, mean=None, rstd=None, out="fp32"):
    """x [R, C]: the values the kernel normalised (after any pre-add).  out: the type y was stored in
    ("bf16", "fp32", or None: y is the fp32 value before the store).  -> {name: ratio per row}"""
    x64, gam, bet = np.asarray(x, F64), np.asarray(gamma, F64), np.asarray(beta, F64)
    C = x64.shape[1]
    ry, rm, rr = fwd64(x64, gam, bet, eps)
    dmu = U * depth(C) * np.abs(x64).max(axis=1)  # the bound on the fp32 mean's error
    res = {}
    if mean is not None:
        res["mean"] = _ratio(np.abs(np.asarray(mean, F64) - rm), U * np.abs(rm) + C_MEAN * dmu)
    if rstd is not None:
        res["rstd"] = _ratio(np.abs(np.asarray(rstd, F64) - rr) / rr, C_RSTD * (8 * U + (rr * dmu) ** 2))
    if y is not None:
        gx = np.abs(ry - bet)
        tol = _rnd(ry, out) + 4 * U * (gx + np.abs(bet)) + C_Y * np.abs(gam) * (rr * dmu)[:, None]
        res["y"] = _ratio(np.abs(np.asarray(y, F64) - ry), tol).max(axis=1)
    return res


def check_bwd(x, dy, gamma, eps, dx=None, dgamma=None, dbeta=None, addend=None, dg0=None, db0=None, out="fp32",
              dy_err=None):
    """dy [R, C] float64 or exact storage values; dy_err: a bound on each element's error where the kernel
    formed dy itself (the fused GEMM).  -> {"dx": ratio per row, "dgamma" / "dbeta": ratio per column}"""
    x64, dy64, gam = np.asarray(x, F64), np.asarray(dy, F64), np.asarray(gamma, F64)
    R, C = x64.shape
    rdx, rdg, rdb = bwd64(x64, dy64, gam, eps, addend, dg0, db0)
    _, rm, rr = fwd64(x64, gam, 0 * gam, eps)
    xh = (x64 - rm[:, None]) * rr[:, None]
    dmu = U * depth(C) * np.abs(x64).max(axis=1)
    g = dy64 * gam
    res = {}
    if dx is not None:
        s1, s2 = g.mean(axis=1)[:, None], (g * xh).mean(axis=1)[:, None]
        add = 0 if addend is None else np.abs(np.asarray(addend, F64))
        rs = rr[:, None]
        tol = _rnd(rdx, out) + 4 * U * (np.abs(rs * g) + np.abs(rs * s1) + np.abs(rs * xh * s2) + add)
        amp = (rr * np.abs(g).max(axis=1) * (1 + np.abs(xh).max(axis=1)) * U * depth(C) * (1 + rr * np.abs(x64).max(axis=1)))
        tol = tol + C_DX * amp[:, None] * (1 + np.abs(xh))
        if dy_err is not None:
            ge = np.abs(gam) * np.asarray(dy_err, F64)
            tol = tol + rs * (ge + ge.max(axis=1)[:, None] * (1 + np.abs(xh) * np.abs(xh).max(axis=1)[:, None]))
        res["dx"] = _ratio(np.abs(np.asarray(dx, F64) - rdx), tol).max(axis=1)
    extra = 0 if dy_err is None else np.asarray(dy_err, F64)
    if dgamma is not None:
        tol = (2.0 ** -23 * np.abs(rdg) + (np.abs(xh) * extra).sum(axis=0) if dy_err is not None
               else 2.0 ** -23 * np.abs(rdg))
        tol = tol + C_DG * (math.sqrt(R) * U * np.abs(dy64 * xh).sum(axis=0)
                            + (np.abs(dy64) * (rr * dmu)[:, None]).sum(axis=0))
        if dg0 is not None:
            tol = tol + U * np.abs(np.asarray(dg0, F64))
        res["dgamma"] = _ratio(np.abs(np.asarray(dgamma, F64) - rdg), tol)
    if dbeta is not None:
        tol = 2.0 ** -23 * np.abs(rdb) + C_DG * math.sqrt(R) * U * np.abs(dy64).sum(axis=0)
        if dy_err is not None:
            tol = tol + extra.sum(axis=0)
        if db0 is not None:
            tol = tol + U * np.abs(np.asarray(db0, F64))
        res["dbeta"] = _ratio(np.abs(np.asarray(dbeta, F64) - rdb), tol)
    return res


def check_gelu_of_ln(x, gamma, beta, eps, post, out, y_out=None, x_err=None):
    """post = gelu(LN(x)) stored in `out`; y_out: the type y was rounded to before the GELU (None: not
    rounded).  |gelu'| <= 1.13, so y's tolerance passes through with that factor.  x_err [R]: a bound on
    the error of each element of the kernel's own x (it reaches y as gamma rstd dx, directly and through
    the mean and the variance).  -> ratio per row"""
    x64, gam, bet = np.asarray(x, F64), np.asarray(gamma, F64), np.asarray(beta, F64)
    C = x64.shape[1]
    ry, _, rr = fwd64(x64, gam, bet, eps)
    dmu = U * depth(C) * np.abs(x64).max(axis=1)
    ty = _rnd(ry, y_out) + 4 * U * (np.abs(ry - bet) + np.abs(bet)) + C_Y * np.abs(gam) * (rr * dmu)[:, None]
    if x_err is not None:
        xh = np.abs(ry - bet) / np.maximum(np.abs(gam), 1e-300)
        ty = ty + np.abs(gam) * (rr * np.asarray(x_err, F64))[:, None] * (2 + xh * xh.max(axis=1)[:, None])
    rp = gelu64(ry)
    tol = _rnd(rp, out) + 4 * U * np.abs(rp) + 1.13 * ty
    return _ratio(np.abs(np.asarray(post, F64) - rp), tol).max(axis=1)


def worst(ratios, names=None):
    """(max ratio, "regime[row]" of it) for messages and the recorded maxima"""
    r = np.asarray(ratios, F64)
    r = np.where(np.isnan(r), np.inf, r)
    i = int(r.argmax())
    return float(r[i]), (f"{names[i]}[{i}]" if names is not None else f"[{i}]")


def by_regime(ratios, names):
    """{regime: max ratio over its rows}"""
    r = np.where(np.isnan(ratios), np.inf, np.asarray(ratios, F64))
    return {n: float(max(v for v, m in zip(r, names) if m == n)) for n in dict.fromkeys(names)}
