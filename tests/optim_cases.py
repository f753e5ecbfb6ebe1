"""Cases, references and the fp32 model of the optimizer step (csrc/optim.hip s2h_grad_norm / s2h_adamw, whose
arithmetic is csrc/optim_elem.h).  Not a test file: test_optim_host.py and test_optim_gpu.py share it.

* `reference_step`: clip_grad_norm_ + torch.optim.AdamW in float64 (numpy).  The betas, eps, max_norm and
  grad_scale it is given are the fp32 values the C ABI carries (`abi`), lr and weight decay are the configuration's
  doubles; with `decay32` the decay scalar is float32(1 - lr * wd) formed in double, as torch applies it to an
  fp32 parameter.
* `model_*`: optim_elem.h operation for operation in numpy fp32.  fmaf is emulated exactly (this Python has no
  math.fma): the product of two fp32 values is exact in float64, the sum is formed with TwoSum, a non-zero error
  is folded into the sticky bit (round to odd), and the 53-bit result is rounded once to fp32.
* `MUTANTS`: named wrong formulas for the model, used on the CPU only to show that the cases tell them apart.
* `model_sumsq`: the summation tree of sumsq_kernel + norm_finalize_kernel in fp32 (products rounded, where the
  compiled kernel may fuse them: the bound of `norm_depth` holds either way), and `norm_depth`, the worst-case
  number of roundings an element's square passes on its way to out[0].
"""
import math

import numpy as np

F = np.float32
N_BIG = 9 * 2 ** 20 + 1203
SIZES = [1, 3, 4, 5, 1023, 4099]
NORM_BLOCKS, BLOCK = 1024, 256
PASS = NORM_BLOCKS * BLOCK * 4  # elements one pass of sumsq_kernel's 16-B loop covers (2^20)
assert PASS == 2 ** 20 and N_BIG < 2 ** 24


def abi(x):
    """the value a `float` argument of the C ABI carries, as a double"""
    return float(F(x))


# ------------------------------------------------------------------------------------------------ exact fmaf
def fmaf(a, b, c):
    """round_fp32(a * b + c) with one rounding, element-wise (fp32 in, fp32 out)"""
    a, b, c = (np.asarray(x, F).astype(np.float64) for x in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b  # exact: 48 significant bits, exponent well inside float64
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)  # TwoSum: p + c == s + err exactly
        odd = (s.view(np.int64) & 1) == 1
        fix = np.isfinite(s) & (err != 0) & ~odd
        toward = np.where(err > 0, np.inf, -np.inf)
        s = np.where(fix, np.nextafter(s, toward), s)  # round to odd: the neighbour with the sticky bit set
        return s.astype(F)


def bf16_bits(x):
    """fp32 -> bf16 bits, round to nearest even (NaN: 0x7fc0, as the host check writes it)"""
    u = np.asarray(x, F).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    return np.where(np.isnan(x), np.uint16(0x7FC0), r)


# ------------------------------------------------------------------------------------------------ the model
def model_scalars(lr, beta1, beta2, wd, step, mutant=None):
    """step_size, bc2_sqrt, decay, w1, omb2 of optim_elem.h from the ABI's floats"""
    lr, beta1, beta2, wd = F(lr), F(beta1), F(beta2), F(wd)
    bc1 = 1.0 - math.pow(float(beta1), float(step))
    bc2 = 1.0 - math.pow(float(beta2), float(step))
    if mutant == "no_bc1":
        bc1 = 1.0
    with np.errstate(all="ignore"):
        step_size = F(np.float64(float(lr)) / np.float64(bc1))
    bc2_sqrt = F(bc2) if mutant == "bc2_not_rooted" else F(math.sqrt(bc2))
    decay = fmaf(-lr, wd, F(1.0))[()]
    if mutant == "l2_coupled":
        decay = F(1.0)
    return dict(step_size=step_size, bc2_sqrt=bc2_sqrt, decay=F(decay), w1=F(1.0) - beta1, omb2=F(1.0) - beta2)


def model_clip_pair(sumsq, max_norm, grad_scale, mutant=None):
    """oe_clip_pair: (out[0], out[1]) from the fp32 sum of squares"""
    with np.errstate(all="ignore"):
        gs, mx = F(grad_scale), F(max_norm)
        root = np.sqrt(F(sumsq))
        norm = root * gs
        used = norm
        if mutant == "scale_missing_from_norm":
            used = root
        elif mutant == "scale_twice_in_norm":
            used = norm * gs
        c = F(1.0)
        if mx > 0:
            c = mx / (used if mutant == "no_1e-6" else used + F(1e-6))
            if c > 1 and mutant != "no_clamp":
                c = F(1.0)
        return F(norm), F(c * gs)


def model_clip_factor(norm, max_norm, grad_scale):
    """out[1] from out[0], the second half of oe_clip_pair"""
    with np.errstate(all="ignore"):
        c = F(1.0)
        if F(max_norm) > 0:
            c = F(max_norm) / (F(norm) + F(1e-6))
            if c > 1:
                c = F(1.0)
        return F(c * F(grad_scale))


def model_adamw(p, g, m, v, cf, sc, beta2, eps, mutant=None, wd=0.0):
    """adamw_elem on arrays: returns (p, m, v) in fp32"""
    p, g, m, v = (np.asarray(x, F) for x in (p, g, m, v))
    cf, beta2, eps = F(cf), F(beta2), F(eps)
    with np.errstate(all="ignore"):
        gi = g * cf
        if mutant == "l2_coupled":
            gi = fmaf(F(wd), p, gi)
        d = fmaf(g, cf, -m) if mutant == "contracted" else gi - m
        mi = fmaf(sc["w1"], d, m)
        vi = fmaf(sc["omb2"], gi * gi, v * beta2)
        if mutant == "eps_before_bc2":
            denom = (np.sqrt(vi) + eps) / sc["bc2_sqrt"]
        elif mutant == "eps_under_sqrt":
            denom = np.sqrt(vi + eps) / sc["bc2_sqrt"]
        else:
            denom = np.sqrt(vi) / sc["bc2_sqrt"] + eps
        if mutant == "decay_after_update":
            po = fmaf(-sc["step_size"], mi / denom, p) * sc["decay"]
        else:
            po = fmaf(-sc["step_size"], mi / denom, p * sc["decay"])
    return po, mi, vi


MUTANTS = ["eps_before_bc2", "eps_under_sqrt", "bc2_not_rooted", "no_bc1", "l2_coupled", "decay_after_update",
           "no_1e-6", "no_clamp", "scale_missing_from_norm", "scale_twice_in_norm", "contracted"]
CLIP_MUTANTS = {"no_1e-6", "no_clamp", "scale_missing_from_norm", "scale_twice_in_norm"}


# ------------------------------------------------------------------------------------------------ the norm's tree
def _wave_block_sum(acc):
    """[blocks, 256] per-thread values -> [blocks]: the xor butterfly of wave_sum over 64 lanes, then
    red[0] + red[1] + red[2] + red[3]"""
    a = acc.reshape(-1, 4, 64)
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        a = a + a[:, :, idx ^ o]
    r = a[:, :, 0]
    return ((r[:, 0] + r[:, 1]) + r[:, 2]) + r[:, 3]


def model_sumsq(x, aligned=True):
    """the fp32 value norm_finalize_kernel takes the root of, in the kernels' summation order"""
    x = np.asarray(x, F)
    n = x.size
    T = NORM_BLOCKS * BLOCK
    with np.errstate(all="ignore"):
        if aligned:
            n4 = n // 4
            sq = x[:4 * n4].reshape(n4, 4)
            sq = sq * sq
            grp = ((sq[:, 0] + sq[:, 1]) + sq[:, 2]) + sq[:, 3]
            rows = -(-n4 // T) if n4 else 0
            grid = np.zeros((max(rows, 1), T), F)
            live = np.zeros((max(rows, 1), T), bool)
            grid.reshape(-1)[:n4] = grp
            live.reshape(-1)[:n4] = True
            a = np.zeros((4, T), F)
            r = 0
            while r + 3 < rows and live[r + 3].any():  # a thread unrolls while its fourth load is inside
                full = live[r + 3]
                for u in range(4):
                    a[u] = np.where(full, a[u] + grid[r + u], a[u])
                tail = ~full
                for u in range(4):  # the other threads go on one load at a time into a[0]
                    a[0] = np.where(tail & live[r + u], a[0] + grid[r + u], a[0])
                r += 4
            for rr in range(r, rows):
                a[0] = np.where(live[rr], a[0] + grid[rr], a[0])
            acc = (a[0] + a[1]) + (a[2] + a[3])
            k = n & 3
            if k:
                t = x[4 * n4:]
                acc[:k] = acc[:k] + t * t
        else:
            rows = -(-n // T)
            grid = np.zeros((rows, T), F)
            grid.reshape(-1)[:n] = x * x
            acc = np.zeros(T, F)
            for rr in range(rows):
                acc = acc + grid[rr]  # + 0 leaves a value unchanged: threads past the end
        part = _wave_block_sum(acc.reshape(NORM_BLOCKS, BLOCK))
        acc = np.zeros(BLOCK, F)
        for i in range(0, NORM_BLOCKS, BLOCK):
            acc = acc + part[i:i + BLOCK]
        return F(_wave_block_sum(acc.reshape(1, BLOCK))[0])


def norm_depth(n, aligned=True):
    """Worst-case number of fp32 roundings between one element and out[0], counted along the kernels' tree.
    sumsq_kernel, 16-B path: the square (1), the three additions inside a float4 (3), the per-lane chain -- lane 0
    has the most loads, U unrolled rounds (one addition each into its accumulator) and R single loads into a[0] --
    (U + R), the accumulator merge (a0 + a1) + (a2 + a3) (2), the scalar tail's addition (1), the wave butterfly
    (6) and red[0..3] (3).  Scalar path: the square (1; none where the compiler fuses it) and a chain of
    ceil(n / 2^18) additions, then 6 + 3.  norm_finalize_kernel: 1024 partials over 256 threads (4), butterfly (6),
    red (3).  The sum of squares has only positive terms, so its relative error is at most depth * 2^-24 to first
    order; the root halves it; sqrtf and the product with grad_scale add one rounding each, and one more covers
    the second-order terms: ceil(depth / 2) + 3 roundings of 2^-24 on out[0]."""
    T = NORM_BLOCKS * BLOCK
    if aligned:
        loads = -(-(n // 4) // T)
        U = 0
        while 4 * U + 3 < loads:
            U += 1
        chain = U + (loads - 4 * U)
        depth = 1 + 3 + chain + 2 + 1 + 6 + 3
    else:
        depth = 1 + -(-n // T) + 6 + 3
    depth += 4 + 6 + 3
    return -(-depth // 2) + 3


def norm_tolerance(n, aligned=True):
    """relative bound on out[0] against the float64 norm"""
    return norm_depth(n, aligned) * 2.0 ** -24


def norm_underflow(n):
    """absolute bound on what the sum of squares loses to underflow: a square below 2^-126 is rounded to a multiple
    of 2^-149 (at most 2^-150 off; sums of such values are exact), so n * 2^-150 -- doubled here.  Over 2 * norm
    it is the norm's share: tests allow norm_tolerance * norm + norm_underflow / norm."""
    return n * 2.0 ** -149


# ------------------------------------------------------------------------------------------------ float64 reference
def reference_clip(g, max_norm, grad_scale):
    """(total norm, factor applied to the stored gradient) of clip_grad_norm_ on grad_scale * g, float64"""
    with np.errstate(all="ignore"):
        gs = np.asarray(g, np.float64) * grad_scale
        total = float(np.sqrt(np.sum(gs * gs)))
        coef = 1.0
        if max_norm > 0:
            coef = max_norm / (total + 1e-6)
            if coef > 1.0:  # clamp(max=1): a NaN stays a NaN
                coef = 1.0
        return total, coef * grad_scale


def reference_adamw(p, gc, m, v, lr, beta1, beta2, eps, wd, step, decay32=True):
    """torch.optim.AdamW's single-tensor step in float64 on the clipped gradient gc: returns (p, m, v)"""
    p, gc, m, v = (np.asarray(x, np.float64) for x in (p, gc, m, v))
    with np.errstate(all="ignore"):
        decay = 1.0 - lr * wd
        if decay32:
            decay = float(F(decay))
        p = p * decay
        m = m + (gc - m) * (1.0 - beta1)
        v = beta2 * v + (1.0 - beta2) * gc * gc
        bc1 = 1.0 - beta1 ** step
        bc2 = 1.0 - beta2 ** step
        denom = np.sqrt(v) / math.sqrt(bc2) + eps
        p = p - (lr / bc1) * (m / denom)
    return p, m, v


def reference_step(case, k, p, m, v, decay32=True):
    """one step of the reference from the fp32 state (p, m, v): returns (norm, factor, p, m, v) in float64"""
    g = case_grad(case, k)
    total, factor = reference_clip(g, abi(case["max_norm"]), abi(case["grad_scale"]))
    with np.errstate(all="ignore"):
        gc = g.astype(np.float64) * factor
    out = reference_adamw(p, gc, m, v, case["lr"], abi(case["beta1"]), abi(case["beta2"]), abi(case["eps"]),
                          case["wd"], case["step0"] + k, decay32)
    return (total, factor) + out


def model_step(case, k, p, m, v, mutant=None, clip_pair=None, aligned=True):
    """one step of the fp32 model: returns (norm, factor, p, m, v).  clip_pair: the device's (out[0], out[1])
    instead of the model's own"""
    g = case_grad(case, k)
    if clip_pair is None:
        clip_pair = model_clip_pair(model_sumsq(g, aligned), case["max_norm"], case["grad_scale"],
                                    mutant if mutant in CLIP_MUTANTS else None)
    sc = model_scalars(case["lr"], case["beta1"], case["beta2"], case["wd"], case["step0"] + k, mutant)
    out = model_adamw(p, g, m, v, clip_pair[1], sc, case["beta2"], case["eps"], mutant, case["wd"])
    return tuple(clip_pair) + out


# ------------------------------------------------------------------------------------------------ error units
def ulp32(x):
    """spacing of fp32 at |x| (the denormal spacing 2^-149 below the normal range)"""
    with np.errstate(all="ignore"):
        return np.spacing(np.abs(np.asarray(x, np.float64)).astype(F)).astype(np.float64)


def error_units(got, ref, before):
    """|got - ref| in units of ulp(ref) + 2^-23 * |ref - before|, element-wise; non-finite references count 0"""
    got, ref, before = (np.asarray(x, np.float64) for x in (got, ref, before))
    with np.errstate(all="ignore"):
        unit = ulp32(ref) + 2.0 ** -23 * np.abs(ref - before)
        e = np.abs(got - ref) / unit
    return np.where(np.isfinite(ref) & np.isfinite(got), e, 0.0)


# ------------------------------------------------------------------------------------------------ the cases
def _weights(n, rng):
    """|p| from 1e-6 to 30, both signs, with exact +0, -0 and 1e-6 and 30 themselves"""
    mag = 10.0 ** rng.uniform(-6.0, math.log10(30.0), n)
    p = (mag * rng.choice([-1.0, 1.0], n)).astype(F)
    for i, val in enumerate((0.0, -0.0, 1e-6, 30.0, -30.0)):
        if n > 8:
            p[(i * 7 + 3) % n] = val
    return p


GRAD_SCALES = [1.0, 1e-4, 1e-8, 1e-12, 1e-20]
DECAY_TIE_LR = 151.5 * 2.0 ** -24 / 0.01  # 9.03e-4: 1 - lr * 0.01 halfway between two fp32 values


def _grad(n, rng, pattern, scale):
    z = rng.standard_normal(n)
    if pattern == "randn":
        g = z * scale
    elif pattern == "zeros":  # exact zeros against (possibly) non-zero moments, every second element
        g = np.where(np.arange(n) % 2 == 0, 0.0, z * scale)
    elif pattern == "mixed":  # every magnitude of GRAD_SCALES and exact zeros in one tensor
        s = np.asarray(GRAD_SCALES + [0.0])[np.arange(n) % (len(GRAD_SCALES) + 1)]
        g = z * s * scale
    elif pattern == "zero":
        g = np.zeros(n)
    else:
        raise ValueError(pattern)
    return g.astype(F)


def case_grad(case, k):
    """the stored gradient of step k (0-based) of a case: a pure function of the case"""
    if "grad_fn" in case:
        return case["grad_fn"](k)
    rng = np.random.default_rng(case["seed"] * 1000 + k)
    g = _grad(case["n"], rng, case["pattern"], case["gscale"])
    if case["n"] > 8:
        g[2::13] = 0.0  # the all-zero elements of _case
    if case.get("poison") is not None and k == 0:
        g[case["poison_at"]] = case["poison"]
    return g


def _case(name, n, seed, *, steps=1, step0=1, state="zero", pattern="randn", gscale=1.0, lr=1e-3, wd=0.01,
          beta1=0.9, beta2=0.999, eps=1e-8, max_norm=1.0, grad_scale=1.0, **extra):
    rng = np.random.default_rng(seed)
    p = _weights(n, rng)
    if state == "zero":
        m, v = np.zeros(n, F), np.zeros(n, F)
    else:  # carried in from a checkpoint: moments of the gradient's magnitude, v >= 0, some of them exact zeros
        s = gscale if pattern != "zero" else 1e-3
        m = (0.3 * s * rng.standard_normal(n)).astype(F)
        v = ((s * rng.standard_normal(n)) ** 2).astype(F)
        if n > 8:
            m[5::11] = 0.0
            v[5::11] = 0.0
    if n > 8:  # elements where everything is zero: they must stay +0
        for a in (p, m, v):
            a[2::13] = 0.0
    c = dict(name=name, n=n, seed=seed, steps=steps, step0=step0, pattern=pattern, gscale=gscale, lr=lr, wd=wd,
             beta1=beta1, beta2=beta2, eps=eps, max_norm=max_norm, grad_scale=grad_scale, p=p, m=m, v=v)
    c.update(extra)
    return c


def make_cases():
    """the AdamW cases (each also runs the clip that precedes it), smallest sizes that reach every path"""
    cs = []
    n = 4099
    for i, s in enumerate(GRAD_SCALES):  # five steps from zero state; scale 1 clips, the others take the clamp
        cs.append(_case(f"zero-state-g{s:g}", n, 10 + i, steps=5, gscale=s))
    for i, step0 in enumerate((1000, 20_000, 200_000)):  # state carried in, bias correction late in a run
        cs.append(_case(f"carried-{step0}-mixed", n, 20 + i, steps=2, step0=step0, state="carried", pattern="mixed"))
        cs.append(_case(f"carried-{step0}-zeros", n, 30 + i, steps=2, step0=step0, state="carried", pattern="zeros",
                        gscale=1e-3))
    cs.append(_case("zero-state-mixed", n, 40, steps=5, pattern="mixed"))
    for i, lr in enumerate((1e-3, 4e-6, 1e-9, 0.0)):  # lr * wd: 1e-5, 4e-8 (just above 2^-25), 1e-11 (below), 0
        for wd in (0.01, 0.0):
            cs.append(_case(f"lr{lr:g}-wd{wd:g}", 1023, 50 + i, steps=2, step0=3, state="carried", lr=lr, wd=wd,
                            gscale=1e-2, max_norm=0.0))
    # float(lr) * float(wd) and the double lr * wd on two sides of a rounding boundary of 1 - lr * wd: the decay
    # scalar is the other fp32 neighbour of torch's
    cs.append(_case("decay-neighbour", 1023, 62, steps=2, step0=3, state="carried", lr=DECAY_TIE_LR, wd=0.01,
                    gscale=1e-2, max_norm=0.0))
    # lr * wd = 1e-2: where the decay is applied (to p before the update, not after) shows beyond the bounds
    cs.append(_case("decay-order", 1023, 63, steps=2, step0=3, state="carried", lr=0.05, wd=0.2, gscale=1e-2,
                    max_norm=0.0))
    cs.append(_case("beta1-0", 1023, 60, steps=2, step0=2, state="carried", beta1=0.0, gscale=1e-2))
    # a clip factor whose products are inexact, against non-zero moments
    cs.append(_case("inexact-clip", n, 61, steps=2, step0=7, state="carried", max_norm=0.0, grad_scale=0.7))
    # the clip's branches, each followed by the update it scales
    cs.append(_case("clip-under", 1023, 70, gscale=1e-3, state="carried", step0=4))       # norm 0.03: the clamp
    cs.append(_case("clip-over", 1023, 71, gscale=1.0, state="carried", step0=4))         # norm 32
    cs.append(_case("clip-tiny-over", 1023, 72, gscale=1e-7, max_norm=1e-6))              # norm 3e-6: the 1e-6 counts
    cs.append(_case("clip-off", 1023, 73, max_norm=0.0, state="carried", step0=4))
    cs.append(_case("clip-zero-grad", 1023, 74, pattern="zero", state="carried", step0=4))
    eq = np.zeros(1023, F)
    eq[[0, 500, 1021, 1022]] = 0.5  # norm exactly 1 = max_norm
    cs.append(_case("clip-equal", 1023, 75, state="carried", step0=4, grad_fn=lambda k, _g=eq: _g.copy()))
    for i, gs in enumerate((0.5, 1.0 / 3.0, 1.0 / 16.0)):
        cs.append(_case(f"scale-{gs:.4f}-over", 1023, 80 + i, grad_scale=gs, state="carried", step0=4))
        cs.append(_case(f"scale-{gs:.4f}-under", 1023, 85 + i, grad_scale=gs, gscale=1e-3, state="carried", step0=4))
    for i, sz in enumerate(SIZES):  # every size: float4 body / tail of 0..3 / a single element
        cs.append(_case(f"size-{sz}", sz, 90 + i, steps=2, step0=2, state="carried", gscale=0.05))
    return cs


def make_big_case():
    """N_BIG elements, one step, a given factor (max_norm 0, grad_scale 0.7): the grid-stride rounds of both kernels"""
    return _case("big", N_BIG, 99, step0=11, state="carried", max_norm=0.0, grad_scale=0.7, gscale=0.02)


def make_nonfinite_cases():
    cs = []
    for i, (tag, val) in enumerate((("inf", np.inf), ("nan", np.nan))):
        for j, mx in enumerate((1.0, 0.0)):
            cs.append(_case(f"{tag}-maxnorm{mx:g}", 1023, 100 + 2 * i + j, state="carried", step0=4, max_norm=mx,
                            poison=val, poison_at=517))
    return cs


def pin_positions(n):
    """where a missed or doubled element would hide: the ends, each side of the float4 tail, each side of every
    multiple of the pass stride"""
    pos = {0, n - 1, 4 * (n // 4) - 1, 4 * (n // 4)}
    for j in range(1, n // PASS + 1):
        pos |= {j * PASS - 1, j * PASS}
    return sorted(q for q in pos if 0 <= q < n)


def pin_tensor(n):
    """zeros with 2^k, k = 0..11 in turn, at pin_positions: returns (g, the exact integer sum of squares)"""
    g = np.zeros(n, F)
    total = 0
    for i, q in enumerate(pin_positions(n)):
        g[q] = 2.0 ** (i % 12)
        total += 4 ** (i % 12)
    assert total < 2 ** 24
    return g, total
