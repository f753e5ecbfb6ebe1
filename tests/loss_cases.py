"""Shared by test_loss_merge_host.py and test_loss_merge_gpu.py: the loss and category-merge kernels of
csrc/loss.hip at the values the tracking loop feeds them -- gated-off objects filled with -1024, logits
saturated at +-40 .. +-90, zeros of both signs, target bytes other than 0 and 1 -- with float64 models of
the operations, an fp32 model of the kernels' own arithmetic (one exponential per pixel), and the checks
both test files run.

A check drives a backend (the fp32 model here, the HIP kernels in the GPU file) through one operation and
returns {assertion name: error / tolerance}; 0 or inf for the exact assertions.  An assertion holds when
its ratio is <= 1.  The host file proves that the clean fp32 model holds every assertion and that each
switchable defect of the model breaks a named one by more than 10x, so the cases can fail.

Tolerances, always against the float64 model:
  integer-valued statistics and selections: exact;
  sums: |got - ref| <= 2e-5 |ref| + 1e-6, per row, on the row's own value;
  gradients: 2e-5 of the row's maximum, plus 1e-12;
  backward coefficients: 2e-5 |ref| + 1e-12 per element (each is a quotient of at most three of the sums,
  which the fp32 model holds to 1e-7; an absolute term as large as the sums' would hide Dice B, ~5e-5).
No summation chain of the kernels is longer than about 40 fp32 roundings (16 per thread, 6 per wave, 4 per
workgroup, then the chunk sums): ~40 * 6e-8 = 2.4e-6 worst case, 1e-7 typical.

Not asserted: merge weights of a category whose every pixel lies in roughly (-104, -87).  There the fp32
sigmoid is denormal: torch keeps that mass, the hardware exponential may flush it to 0, and the category
then takes the plain-mean branch on one side only."""
import functools
import math

import torch
import torch.nn.functional as F

NSTAT = 6
NO_OBJ = -1024.0  # NO_OBJ_SCORE: what row_gate writes into a gated-off object
ROW_GATED, ROW_EMPTY, ROW_RIGHT, ROW_WRONG, ROW_ZEROS, ROW_WIDE, ROW_FULL = 1, 2, 3, 4, 5, 6, 7
ZERO_VALUES = [0.0, -0.0, 1e-30, -1e-30, 1e-3, -1e-3]
SET_BYTES = [1, 2, 255]
WEIGHTS = (20.0, 1.0, 1.0)
INV_TEMPS = [1.0, 1.0 / 0.7]
F32, F64 = torch.float32, torch.float64


def f32(v):
    """the value a C float argument takes"""
    return float(torch.tensor(v, dtype=F32))


# ------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def make_rows(P, seed=0):
    """logits [8, P] fp32 and targets [8, P] uint8, one row per regime (shared: do not write into them)"""
    g = torch.Generator().manual_seed(1000 * seed + P)
    x = torch.empty(8, P, dtype=F32)
    on = torch.zeros(8, P, dtype=torch.bool)

    def frac(f, row):
        m = torch.rand(P, generator=g) < f
        m[row % P] = True  # never empty, whatever P
        return m

    x[0] = torch.randn(P, generator=g) * 3
    on[0] = frac(0.3, 0)
    x[ROW_GATED] = NO_OBJ
    on[ROW_GATED] = frac(0.2, 1)
    x[ROW_EMPTY] = torch.randn(P, generator=g) * 3
    for r in (ROW_RIGHT, ROW_WRONG, ROW_ZEROS, ROW_WIDE):
        on[r] = frac(0.5, r)
    x[ROW_RIGHT] = torch.where(on[ROW_RIGHT], 40.0, -40.0)
    x[ROW_WRONG] = torch.where(on[ROW_WRONG], -40.0, 40.0)
    x[ROW_ZEROS] = torch.tensor(ZERO_VALUES, dtype=F32)[torch.randint(0, 6, (P,), generator=g)]
    x[ROW_ZEROS, 0] = 0.0  # x == 0 under a set target: background for the IoU count
    on[ROW_ZEROS, 0] = True
    if P > 1:
        x[ROW_ZEROS, 1] = -0.0
        on[ROW_ZEROS, 1] = True
    x[ROW_WIDE] = torch.rand(P, generator=g) * 180 - 90
    x[ROW_FULL] = -NO_OBJ
    on[ROW_FULL] = True
    byte = torch.tensor(SET_BYTES, dtype=torch.uint8)[torch.randint(0, 3, (8, P), generator=g)]
    t = torch.where(on, byte, torch.zeros((), dtype=torch.uint8))
    return x, t


@functools.lru_cache(maxsize=None)
def pred_ious(P, seed=0):
    g = torch.Generator().manual_seed(77 + seed)
    return torch.rand(8, generator=g, dtype=F32)


class Groups:
    def __init__(self, obj_to_cat, ncat):
        self.obj_to_cat, self.ncat = list(obj_to_cat), ncat
        self.members = [[o for o, c in enumerate(obj_to_cat) if c == k] for k in range(ncat)]


# objects 0..7 of the merge cases = rows OBJ_ROWS of make_rows; categories: 0 empty, 1 one live object,
# 2 two gated-off objects (zero mass: the mean branch), 3 three live objects whose sigmoid has a slope
# (weighted), 4 a live object beside a gated-off one
OBJ_ROWS = [ROW_RIGHT, ROW_GATED, ROW_GATED, 0, ROW_ZEROS, ROW_FULL, ROW_GATED, ROW_WIDE]
GROUPS = Groups([1, 2, 2, 3, 3, 4, 4, 3], 5)
CAT_EMPTY, CAT_ONE, CAT_GATED, CAT_WEIGHTED, CAT_MIXED = range(5)


@functools.lru_cache(maxsize=None)
def make_objects(P, seed=0):
    """clean object logits [8, P] (the merge weights come from them)"""
    return make_rows(P, seed)[0][OBJ_ROWS].clone()


@functools.lru_cache(maxsize=None)
def make_max_objects(P, seed=0):
    """make_objects with the selection edges written into category 3 (objects 3, 4, 7): zeros of both signs,
    one NaN, two NaNs, a column of -inf"""
    x = make_objects(P, seed).clone()
    inf, nan = float("inf"), float("nan")
    edits = [(0, (0.0, -0.0, -5.0)), (1, (-0.0, 0.0, -5.0)), (2, (1.0, nan, 2.0)), (3, (nan, 0.0, nan)),
             (4, (-inf, -inf, -inf)), (5, (7.5, 7.5, 7.5))]
    for p, vals in edits:
        if p < P:
            for o, v in zip((3, 4, 7), vals):
                x[o, p] = v
    return x


def zero_tie_columns(x, groups):
    """[ncat, P] bool: the category's maximum is a zero that objects hold with both signs"""
    out = torch.zeros(groups.ncat, x.shape[1], dtype=torch.bool)
    for c, m in enumerate(groups.members):
        if m:
            z = x[m] == 0
            neg = torch.signbit(x[m])
            top = x[m].max(0).values == 0
            out[c] = top & (z & neg).any(0) & (z & ~neg).any(0)
    return out


# ------------------------------------------------------------------ float64 models
def ce64(x, t):
    """binary cross-entropy with logits: -(t log sigma(x) + (1 - t) log sigma(-x))"""
    return -(t * F.logsigmoid(x) + (1 - t) * F.logsigmoid(-x))


def _rows64(x, t, inv_temp):
    xv = x.double() * inv_temp
    tb = torch.zeros_like(xv) if t is None else (t != 0).double()
    return xv, tb


def stats64(x, t, inv_temp=1.0):
    """[N, 6]: focal sum, sigmoid sum, target sum, sigmoid . target sum, |pred & gt|, |pred | gt|"""
    xv, tb = _rows64(x, t, inv_temp)
    s = torch.sigmoid(xv)
    pt = s * tb + (1 - s) * (1 - tb)
    focal = (0.25 * tb + 0.75 * (1 - tb)) * ce64(xv, tb) * (1 - pt) ** 2
    pred, gt = xv > 0, tb > 0
    return torch.stack([focal.sum(1), s.sum(1), tb.sum(1), (s * tb).sum(1), (pred & gt).sum(1).double(),
                        (pred | gt).sum(1).double()], 1)


def frame64(x, t, pred_iou, valid, weights=WEIGHTS, inv_temp=1.0):
    """one frame's [mask, dice, iou, total] as a differentiable float64 tensor.  valid: explicit flags, or
    None for target sum > 0.  A frame with no valid row gives zeros (the project being rebuilt raises)."""
    xv, tb = _rows64(x, t, inv_temp)
    s = torch.sigmoid(xv)
    pt = s * tb + (1 - s) * (1 - tb)
    lm = ((0.25 * tb + 0.75 * (1 - tb)) * ce64(xv, tb) * (1 - pt) ** 2).mean(1)
    ld = 1 - (2 * (s * tb).sum(1) + 1) / (s.sum(1) + tb.sum(1) + 1)
    pred, gt = xv.detach() > 0, tb > 0
    actual = (pred & gt).sum(1).double() / (pred | gt).sum(1).double().clamp(min=1.0)
    li = (pred_iou.double() - actual).abs()
    v = tb.sum(1) > 0 if valid is None else torch.as_tensor(valid) != 0
    nv = int(v.sum())
    if nv == 0:
        zero = xv.sum() * 0 + pred_iou.double().sum() * 0
        return torch.stack([zero, zero, zero, zero])
    parts = [q[v].sum() / nv for q in (lm, ld, li)]
    return torch.stack(parts + [weights[0] * parts[0] + weights[1] * parts[1] + weights[2] * parts[2]])


def frame_grads64(x, t, pred_iou, valid, weights=WEIGHTS, inv_temp=1.0, scale=1.0):
    """scale * d total / d logits [N, P] and scale * d total / d pred_iou [N], by autograd"""
    xd = x.double().clone().requires_grad_(True)
    pd = pred_iou.double().clone().requires_grad_(True)
    total = frame64(xd, t, pd, valid, weights, inv_temp)[3]
    gx, gp = torch.autograd.grad(total, [xd, pd])
    return gx * scale, gp * scale


def coef64(stats, pred_iou, valid, P, weights=WEIGHTS, gscale=1.0):
    """the four backward coefficients per row in closed form from float64 statistics"""
    s = stats.double()
    v = s[:, 2] > 0 if valid is None else torch.as_tensor(valid) != 0
    nv = int(v.sum())
    out = torch.zeros(s.shape[0], 4, dtype=F64)
    if nv == 0:
        return out
    den = s[:, 1] + s[:, 2] + 1
    diff = pred_iou.double() - s[:, 4] / s[:, 5].clamp(min=1.0)
    out[:, 0] = gscale * weights[0] / (nv * P)
    out[:, 1] = gscale * weights[1] * 2 / (nv * den)
    out[:, 2] = gscale * weights[1] * (2 * s[:, 3] + 1) / (nv * den * den)
    out[:, 3] = gscale * weights[2] * torch.sign(diff) / nv
    out[~v] = 0
    return out


def bce_rows64(x, t, pos_weight, inv_temp=1.0):
    """[N, P] elementwise BCE with logits and pos_weight, differentiable"""
    xv, tb = _rows64(x, t, inv_temp)
    w = 1.0 if pos_weight is None else pos_weight.double().view(-1, 1)
    return -(w * tb * F.logsigmoid(xv) + (1 - tb) * F.logsigmoid(-xv))


def bce64(x, t, pos_weight, inv_temp, reduction, frame_scale=1.0):
    """frame_scale * mean (reduction 0) or sum (1) over the rows with target pixels; the mean of nothing is NaN"""
    el = bce_rows64(x, t, pos_weight, inv_temp)
    sel = el[(t != 0).sum(1) > 0]
    return frame_scale * (sel.mean() if reduction == 0 else sel.sum())


def bce_grad64(x, t, pos_weight, inv_temp, reduction, frame_scale=1.0, scale=1.0):
    if not bool(((t != 0).sum(1) > 0).any()):
        return torch.zeros(x.shape, dtype=F64)
    xd = x.double().clone().requires_grad_(True)
    (g,) = torch.autograd.grad(bce64(xd, t, pos_weight, inv_temp, reduction, frame_scale), [xd])
    return g * scale


def group_max_model(x, groups, last_wins=False):
    """pixelwise maximum over each category's objects: the first maximum wins ties, the first NaN wins
    outright; an empty category gives y = 0, arg = -1.  Selection only: exact in any dtype."""
    P = x.shape[1]
    y = torch.zeros(groups.ncat, P, dtype=x.dtype)
    arg = torch.full((groups.ncat, P), -1, dtype=torch.int32)
    for c, objs in enumerate(groups.members):
        for k, o in enumerate(objs):
            v = x[o]
            if k == 0:
                take = torch.ones(P, dtype=torch.bool)
            else:
                take = ((v >= y[c]) if last_wins else (v > y[c])) | (torch.isnan(v) & ~torch.isnan(y[c]))
            y[c] = torch.where(take, v, y[c])
            arg[c] = torch.where(take, torch.full_like(arg[c], o), arg[c])
    return y, arg


def group_max_bwd_model(dy, arg, groups):
    O = len(groups.obj_to_cat)
    dx = torch.zeros(O, dy.shape[1], dtype=dy.dtype)
    for o, c in enumerate(groups.obj_to_cat):
        dx[o] = torch.where(arg[c] == o, dy[c], torch.zeros_like(dy[c]))
    return dx


def wavg64(s, w, groups, zero_mass_weighted=False):
    """y[c] = sum_o w_o s_o / sum_o w_o over the category's objects; their plain mean when sum w == 0; 0 when
    the category is empty.  s [O, K], w [O] (the sigmoid mass), differentiable."""
    rows = []
    for objs in groups.members:
        if not objs:
            rows.append(s.sum(0) * 0)
            continue
        sw = w[objs].sum()
        if float(sw.detach()) == 0.0 and not zero_mass_weighted:
            rows.append(s[objs].mean(0))
        else:
            rows.append((s[objs] * w[objs].view(-1, 1)).sum(0) / sw)
    return torch.stack(rows)


def wavg_grads64(s, hr, dy, groups):
    """y, d<y, dy>/ds [O, K], d<y, dy>/dw [O] and d<y, dy>/d hr [O, P] with w = sum sigmoid(hr), by autograd"""
    sd = s.double().clone().requires_grad_(True)
    hd = hr.double().clone().requires_grad_(True)
    w = torch.sigmoid(hd).sum(1)
    w.retain_grad()
    y = wavg64(sd, w, groups)
    (y * dy.double()).sum().backward()
    zero = lambda g, like: torch.zeros_like(like) if g is None else g  # noqa: E731
    return y.detach(), zero(sd.grad, sd), zero(w.grad, w), zero(hd.grad, hd)


# ------------------------------------------------------------------ fp32 model of the kernels' arithmetic
DEFECTS = ["naive_softplus", "pred_ge", "no_union_clamp", "dice_no_smooth", "valid_from_stats", "last_max_wins",
           "zero_mass_weighted", "bwd_no_inv_temp"]


class KernelModel:
    """csrc/loss.hip in torch fp32 on the CPU: per pixel e = exp(-|x|), r = 1 / (1 + e),
    ce = max(x, 0) - x t + log(1 + e), sigma = x >= 0 ? r : e r.  Each name in `defects` makes exactly one
    change; only the host test sets any."""

    def __init__(self, defects=()):
        assert all(d in DEFECTS for d in defects)
        self.d = set(defects)

    def _pixel(self, x, t, inv_temp):
        xv = x * f32(inv_temp)
        tf = torch.zeros_like(xv) if t is None else (t != 0).float()
        e = torch.exp(-xv.abs())
        r = 1.0 / (1.0 + e)
        if "naive_softplus" in self.d:
            ce = torch.log(1.0 + torch.exp(xv)) - xv * tf
        else:
            ce = xv.clamp(min=0) - xv * tf + torch.log(1.0 + e)
        s = torch.where(xv >= 0, r, e * r)
        return xv, tf, s, ce

    def stats(self, x, t, inv_temp=1.0):
        xv, tf, s, ce = self._pixel(x, t, inv_temp)
        pt = s * tf + (1 - s) * (1 - tf)
        q = 1 - pt
        focal = (0.25 * tf + 0.75 * (1 - tf)) * ce * q * q
        pred = (xv >= 0) if "pred_ge" in self.d else (xv > 0)
        gt = tf > 0
        return torch.stack([focal.sum(1), s.sum(1), tf.sum(1), (s * tf).sum(1), (pred & gt).sum(1).float(),
                            (pred | gt).sum(1).float()], 1)

    def finalize(self, stats, pred_iou, valid, P, weights, gscale, losses):
        one = lambda v: torch.tensor(v, dtype=F32)  # noqa: E731
        wm, wd, wi, gs = (one(v) for v in (*weights, gscale))
        N = stats.shape[0]
        if valid is None or "valid_from_stats" in self.d:
            v = [bool(stats[n, 2] > 0) for n in range(N)]
        else:
            v = [bool(valid[n] != 0) for n in range(N)]
        nv = sum(v)
        inv_nv = one(1.0) / one(float(nv)) if nv else one(0.0)
        coef = torch.zeros(N, 4, dtype=F32)
        lm, ld, li = one(0.0), one(0.0), one(0.0)
        Pf = one(float(P))
        for n in range(N):
            if not v[n]:
                continue
            s = stats[n]
            lm = lm + s[0] / Pf
            if "dice_no_smooth" in self.d:
                den, num = s[1] + s[2], 2 * s[3]
            else:
                den, num = s[1] + s[2] + 1, 2 * s[3] + 1
            ld = ld + (1 - num / den)
            actual = s[4] / (s[5] if "no_union_clamp" in self.d else s[5].clamp(min=1.0))
            diff = pred_iou[n] - actual
            li = li + diff.abs()
            cd = gs * wd * inv_nv
            coef[n, 0] = gs * wm * inv_nv / Pf
            coef[n, 1] = cd * 2 / den
            coef[n, 2] = cd * num / (den * den)
            coef[n, 3] = gs * wi * inv_nv * (1.0 if diff > 0 else (-1.0 if diff < 0 else 0.0))
        lm, ld, li = lm * inv_nv, ld * inv_nv, li * inv_nv
        return losses + torch.stack([lm, ld, li, wm * lm + wd * ld + wi * li]), coef

    def bwd(self, x, t, coef, inv_temp, gtot):
        xv, tf, s, ce = self._pixel(x, t, inv_temp)
        gs = torch.tensor(1.0) if gtot is None else gtot[3]
        ds = s * (1 - s)
        pt = s * tf + (1 - s) * (1 - tf)
        q = 1 - pt
        dfocal = (0.25 * tf + 0.75 * (1 - tf)) * (-2 * q * (2 * tf - 1) * ds * ce + q * q * (s - tf))
        g = coef[:, 0:1] * dfocal - (coef[:, 1:2] * tf - coef[:, 2:3]) * ds
        live = (coef[:, :3] != 0).any(1, keepdim=True)
        g = torch.where(live, g, torch.zeros_like(g))
        it = 1.0 if "bwd_no_inv_temp" in self.d else f32(inv_temp)
        return g * it * gs, coef[:, 3] * gs

    def gmax(self, x, groups):
        return group_max_model(x, groups, last_wins="last_max_wins" in self.d)

    def gmax_bwd(self, dy, arg, groups):
        return group_max_bwd_model(dy, arg, groups)

    def wavg(self, s, stats, groups):
        return wavg64(s, stats[:, 1], groups, zero_mass_weighted="zero_mass_weighted" in self.d)

    def wavg_bwd(self, s, y, dy, stats, groups):
        w = stats[:, 1]
        ds, dw = torch.zeros_like(s), torch.zeros(s.shape[0], dtype=F32)
        for c, objs in enumerate(groups.members):
            if not objs:
                continue
            sw = w[objs].sum()
            for o in objs:
                if float(sw) == 0.0:
                    ds[o] = dy[c] / len(objs)
                else:
                    ds[o] = dy[c] * w[o] / sw
                    dw[o] = (dy[c] * (s[o] - y[c]) / sw).sum()
        return ds, dw

    def sig_axpy(self, hr, coef, dx):
        s = 1.0 / (1.0 + torch.exp(-hr))
        return torch.where(coef.view(-1, 1) != 0, dx + coef.view(-1, 1) * s * (1 - s), dx)


# ------------------------------------------------------------------ error / tolerance ratios
def _worst(err, tol, got, ref):
    bad = ~torch.isfinite(got.double()) | ~torch.isfinite(ref.double())
    same = (torch.isnan(got.double()) & torch.isnan(ref.double())) | (got.double() == ref.double())
    r = torch.where(bad, torch.where(same, 0.0, math.inf), err / tol)
    return float(r.max()) if r.numel() else 0.0


def sum_ratio(got, ref):
    """per element: |got - ref| / (2e-5 |ref| + 1e-6)"""
    g, r = got.double(), ref.double()
    return _worst((g - r).abs(), 2e-5 * r.abs() + 1e-6, g, r)


def rel_ratio(got, ref):
    """per element: |got - ref| / (2e-5 |ref| + 1e-12)"""
    g, r = got.double(), ref.double()
    return _worst((g - r).abs(), 2e-5 * r.abs() + 1e-12, g, r)


def grad_ratio(got, ref):
    """per row: max |got - ref| / (2e-5 max |ref| + 1e-12)"""
    g, r = got.double().reshape(got.shape[0], -1), ref.double().reshape(ref.shape[0], -1)
    if not (bool(torch.isfinite(g).all()) and bool(torch.isfinite(r).all())):
        return math.inf
    return float(((g - r).abs().amax(1) / (2e-5 * r.abs().amax(1) + 1e-12)).max())


def exact(got, ref):
    """0 when equal (NaN == NaN), else inf"""
    return 0.0 if got.shape == ref.shape and bool(((got == ref) | (torch.isnan(got) & torch.isnan(ref))).all()) else math.inf


def same_bits(got, ref):
    """0 when the fp32 bit patterns agree away from NaN and the NaN positions agree, else inf"""
    n = torch.isnan(ref)
    if not torch.equal(torch.isnan(got), n):
        return math.inf
    return 0.0 if torch.equal(got.masked_fill(n, 0).view(torch.int32), ref.masked_fill(n, 0).view(torch.int32)) else math.inf


def failed(ratios):
    """the assertions that do not hold"""
    return {k: v for k, v in ratios.items() if not v <= 1.0}


# ------------------------------------------------------------------ the checks
@functools.lru_cache(maxsize=None)
def _stats_ref(P, inv_temp, with_tgt):
    x, t = make_rows(P)
    return stats64(x, t if with_tgt else None, f32(inv_temp))


def check_mask_stats(be, P, inv_temp=1.0, with_tgt=True):
    x, t = make_rows(P)
    got = be.stats(x, t if with_tgt else None, inv_temp)
    ref = _stats_ref(P, inv_temp, with_tgt)
    out = {"stats.%s" % n: sum_ratio(got[:, k], ref[:, k]) for k, n in ((0, "focal"), (1, "sigma"), (3, "sigma_t"))}
    out.update({"stats.%s" % n: exact(got[:, k].double(), ref[:, k]) for k, n in ((2, "tsum"), (4, "inter"), (5, "union"))})
    return out


def _finalize_case(be, out, name, P, stats, x, t, ious, valid, inv_temp, gscale=1.0, ncoef=4):
    losses, coef = be.finalize(stats, ious, valid, P, WEIGHTS, gscale, torch.zeros(4, dtype=F32))
    it = f32(inv_temp)
    ref = frame64(x, t, ious, valid, WEIGHTS, it).detach()
    cref = coef64(stats64(x, t, it), ious, valid, P, WEIGHTS, f32(gscale))
    out[name + ".losses"] = sum_ratio(losses, ref)
    out[name + ".coef"] = rel_ratio(coef[:, :ncoef], cref[:, :ncoef])
    return losses, coef


def sign_ious(stats):
    """pred_iou equal to, above and below the actual IoU, row by row in turn (fp32, from the exact counts)"""
    actual = stats[:, 4].float() / stats[:, 5].float().clamp(min=1.0)
    step = torch.tensor([0.0, 0.125, -0.125], dtype=F32)[torch.arange(stats.shape[0]) % 3]
    return actual + step, torch.sign(step)


def check_finalize(be, P, inv_temp=1.0):
    x, t = make_rows(P)
    it = f32(inv_temp)
    stats = be.stats(x, t, inv_temp)
    ious = pred_ious(P)
    has = ((t != 0).sum(1) > 0).int()
    out = {}
    # explicit flags equal to target sum > 0, and derived flags: the same numbers
    la, ca = _finalize_case(be, out, "flags", P, stats, x, t, ious, has, inv_temp)
    lb, cb = _finalize_case(be, out, "derived", P, stats, x, t, ious, None, inv_temp)
    out["derived.same_as_flags"] = max(exact(la, lb), exact(ca, cb))
    # an explicit flag on the row without target pixels: the row counts, with Dice 1 - 1 / (sum sigma + 1)
    flagged = has.clone()
    flagged[ROW_EMPTY] = 1
    _, cf = _finalize_case(be, out, "flag_on_empty", P, stats, x, t, ious, flagged, inv_temp)
    out["flag_on_empty.row_counts"] = 0.0 if bool((cf[ROW_EMPTY, :3] != 0).all()) else math.inf
    # no valid row: losses unchanged, coef all zero, everything finite
    before = torch.tensor([0.5, 1.5, 2.5, 3.5], dtype=F32)
    ln, cn = be.finalize(stats, ious, torch.zeros(8, dtype=torch.int32), P, WEIGHTS, 1.0, before.clone())
    out["none_valid.losses_unchanged"] = exact(ln, before)
    out["none_valid.coef_zero"] = exact(cn, torch.zeros(8, 4, dtype=F32))
    # no target at all, every row flagged: the gated-off row has |pred | gt| = 0 and an actual IoU of 0 / max(0, 1)
    s0 = be.stats(x, None, inv_temp)
    ones = torch.ones(8, dtype=torch.int32)
    _finalize_case(be, out, "no_target", P, s0, x, None, ious, ones, inv_temp)
    # two frames into one buffer: the sum
    l1, _ = be.finalize(stats, ious, None, P, WEIGHTS, 1.0, torch.zeros(4, dtype=F32))
    l2, _ = be.finalize(s0, ious, ones, P, WEIGHTS, 1.0, l1.clone())
    ref2 = frame64(x, t, ious, None, WEIGHTS, it).detach() + frame64(x, None, ious, ones, WEIGHTS, it).detach()
    out["two_frames.losses"] = sum_ratio(l2, ref2)
    _finalize_case(be, out, "gscale", P, stats, x, t, ious, None, inv_temp, gscale=0.5)
    # pred_iou equal to, above and below the actual IoU: sign coefficients 0, +1, -1
    si, sg = sign_ious(_stats_ref(P, inv_temp, True))
    # (equal in fp32: the float64 difference there is a rounding error with a sign of its own, so column 3
    # is compared with the intended signs only)
    _, cs = _finalize_case(be, out, "iou_sign", P, stats, x, t, si, ones, inv_temp, ncoef=3)
    out["iou_sign.exact"] = exact(cs[:, 3], sg * f32(WEIGHTS[2]) / 8)
    return out


def check_mask_bwd(be, P, inv_temp=1.0, gs=0.37):
    """gs: gtot[3], or None for no upstream gradient"""
    x, t = make_rows(P)
    it = f32(inv_temp)
    stats = be.stats(x, t, inv_temp)
    ious = pred_ious(P)
    _, coef = be.finalize(stats, ious, None, P, WEIGHTS, 0.5, torch.zeros(4, dtype=F32))
    gtot = None if gs is None else torch.tensor([9.0, 9.0, 9.0, gs], dtype=F32)  # only entry 3 is read
    dx, dious = be.bwd(x, t, coef, inv_temp, gtot)
    scale = f32(0.5) * (1.0 if gs is None else f32(gs))
    rx, ri = frame_grads64(x, t, ious, None, WEIGHTS, it, scale)
    out = {"bwd.dx": grad_ratio(dx, rx), "bwd.dious": rel_ratio(dious.reshape(-1), ri)}
    out["bwd.invalid_rows_zero"] = exact(dx[ROW_EMPTY], torch.zeros(P, dtype=F32))
    # the gated-off row: sigma = 0 exactly, so d focal / dx = -0.25 on set pixels and 0 elsewhere, in fp32 exactly
    # (the two kernels multiply by inv_temp and gs in either order)
    g = coef[ROW_GATED, 0] * -0.25
    gsf = torch.tensor(1.0 if gs is None else gs, dtype=F32)
    itf = torch.tensor(inv_temp, dtype=F32)
    on = t[ROW_GATED] != 0
    row = dx[ROW_GATED]
    forms = [torch.where(on, v, torch.zeros((), dtype=F32)) for v in ((g * itf) * gsf, g * (itf * gsf))]
    out["bwd.gated_row_exact"] = min(exact(row, f) for f in forms)
    return out


def check_group_max(be, P):
    x = make_max_objects(P)
    y, arg = be.gmax(x, GROUPS)
    ry, rarg = group_max_model(x, GROUPS)
    keep = ~zero_tie_columns(x, GROUPS)
    out = {"gmax.y_bits": same_bits(y, ry), "gmax.arg": exact(arg[keep], rarg[keep]),
           "gmax.empty": max(exact(y[CAT_EMPTY], torch.zeros(P)), exact(arg[CAT_EMPTY], torch.full((P,), -1, dtype=torch.int32)))}
    g = torch.Generator().manual_seed(5)
    dy = torch.randn(GROUPS.ncat, P, generator=g)
    dx = be.gmax_bwd(dy, arg, GROUPS)
    out["gmax_bwd.dx"] = exact(dx, group_max_bwd_model(dy, arg, GROUPS))
    cons = 0.0
    for c, objs in enumerate(GROUPS.members):
        if objs:  # one object per pixel holds dy, the others 0: the sum is exact
            cons = max(cons, exact(dx[objs].sum(0), dy[c]), 0.0 if int((dx[objs] != 0).sum(0).max()) <= 1 else math.inf)
    out["gmax_bwd.conserves"] = cons
    return out


def check_wavg(be, P, K):
    hr = make_objects(P)
    g = torch.Generator().manual_seed(11 + K)
    s = torch.rand(8, K, generator=g)
    dy = torch.randn(GROUPS.ncat, K, generator=g)
    dx0 = torch.randn(8, P, generator=g) / P  # the size of the term added into it
    stats = be.stats(hr, None, 1.0)
    y = be.wavg(s, stats, GROUPS)
    ds, dw = be.wavg_bwd(s, y, dy, stats, GROUPS)
    dhr = be.sig_axpy(hr, dw, dx0.clone())
    ry, rds, rdw, rdhr = wavg_grads64(s, hr, dy, GROUPS)
    out = {"wavg.y": sum_ratio(y, ry), "wavg.ds": grad_ratio(ds.reshape(1, -1), rds.reshape(1, -1)),
           "wavg.dw": grad_ratio(dw.reshape(1, -1), rdw.reshape(1, -1)), "wavg.dhr": grad_ratio(dhr, rdhr + dx0.double())}
    gated = GROUPS.members[CAT_GATED]
    out["wavg.zero_mass_is_mean"] = sum_ratio(y[CAT_GATED], s[gated].double().mean(0))
    out["wavg.zero_mass_ds"] = exact(ds[gated], (dy[CAT_GATED] / len(gated)).expand(len(gated), K))
    out["wavg.zero_mass_dw"] = exact(dw[gated], torch.zeros(len(gated)))
    out["wavg.zero_mass_dhr_untouched"] = same_bits(dhr[gated], dx0[gated])
    out["wavg.empty"] = exact(y[CAT_EMPTY], torch.zeros(K))
    return out


def weighted_masses(P):
    """float64 sigmoid mass of every category that takes the weighted branch"""
    w = torch.sigmoid(make_objects(P).double()).sum(1)
    return [float(w[m].sum()) for m in GROUPS.members if m and float(w[m].sum()) != 0.0]
