"""Shared by test_decoder_tok_host.py and test_decoder_tok_kernels_gpu.py: the four token-side kernels of
csrc/decoder_tok.hip (dt_self, dt_post_a, dt_post_b, dt_final behind s2h_dec_self / _post_a / _post_b /
_final), every one of their stored outputs (19 bf16 slots, 8 statistic vectors, lse) pinned to a float64
model of the ONE stage that produced it.

Every intermediate of these kernels is written to a slot, so a stage's reference takes the kernel's own
stored inputs of that stage (bf16 values, exact in float64): no error carries from one stage to the next,
and a flipped bf16 rounding upstream can neither hide nor fake a failure downstream.  Everything here is
numpy; nothing touches a device.

Shapes (T tokens per object, objects), R = T * objects rows, against dt_rows (per = 16 // T objects share a
workgroup, the last workgroup may be partial): SHAPES below.

Operand classes:
  exact    x, pe, ot, x1, of, x3, y3 in {-1, 0, 1}, ternary weights, integer biases in -3 .. 3; max|acc| <= 256
           is asserted on the float64 product, so qs / ks / vs (dt_self), y2 (dt_post_a) and y (dt_final) are
           bf16 integers in any summation order: EQUAL_SLOTS, compared for equality.
  real     randn activations rounded to bf16, weights ~ N(0, 1/K) rounded to bf16, fp32 biases, gamma / beta
           of ln_cases.make_params.
  ln       the row regimes of ln_cases.make_rows(256, "bf16") (offset300, offset30, outlier, const, const_ulp,
           tiny, large, zero, neg_offset; randn too) reach each dt_layernorm: dt_post_b takes them as y3;
           dt_post_a / dt_final through the residual with a zero out-projection and zero bias (y2 = x1,
           y = x3); dt_self with skip = 0, zero Wo and bo (y1 = x).  eps 1e-6 and 1e-5.
  bias300  a real case whose LayerNorm-feeding projection has a bias of 300 + noise: the offset is formed
           inside the launch and its bf16 rounding (spacing 2) is what the statistics must see.  dt_post_b
           has no projection in front of its LayerNorm: there y3 = bf16(300 + randn).
  softmax  dt_self only.  Wq / Wk rows 0..127 are 0/1 selections (q of heads 0..3 = channels 0..127 of
           x + pe, k = channels 128..255), zero bias; rows 128..255 (heads 4..7) are dense real rows (256
           channels cannot feed eight heads' q and k independently).  On the steered heads the scores are
           a_i c_j + shift + noise on a bf16-exact lattice (step 2^-4), regime (object + head) % 4:
           flat (every key of the object the same vector: all scores equal, p = 1/T), peaked (one key ahead
           by >= 100 nats, asserted), shifted by +60 and by -60 nats (with gains up to 6.3 x 6.3 nats on
           top: without the max subtraction exp2f overflows / underflows).  Neighbouring objects -- the
           ones that share a workgroup -- therefore differ in regime, and in v.
Every case runs with skip in {0, 1} (dt_self; with skip = 1 a null qa is passed, and the ln class then
normalises y1 = 0: no residual may arrive) and final_q in {0, 1} (dt_post_b; 0 passes null qfa / qqf / Wqf).

Stage models (float64), u = 2^-24, rnd(v) = 2^-8 |v| (half a bf16 ulp at worst):
  adds     qa = bf16(x + pe), qt = bf16(x1 + pe), q2 = qfa = bf16(x3 + pe): an fp32 sum of two bf16 values
           rounded once is the correctly rounded float64 sum -- equality in every class.
  proj     out = src W^T + b (+ res), PROJ below names src / res of each.  Tolerance per element
           rnd(ref) + C_PROJ K u (sum_k |a_k w_k| + |b| + |res|): an fp32 sum of K products in any order.
  attn     from the stored qs, ks, vs per object, head, query i; delta_i = 32 u scale max_j sum_c |q_ic k_jc|
           bounds a score's error.  lse (natural log, [objects, 8, T]): C_LSE (delta_i + u (|lse| + 4)).
           os: rnd(os) + 2^-8 sum_j p_ij |v_jc| + 2^-126 sum_j |v_jc|
               + C_OS (delta_i sum_j p_ij |v_jc - o_ic| + (3 T + 4) u sum_j p_ij |v_jc|);
           the 2^-8 term is the documented convention (unnormalised P rounded to bf16 for P V, the
           normaliser from the unrounded values).
  ln       x1 / mean1 / rstd1 from the stored y1, x2 from y2, x3 from y3, hs from y: ln_cases.check_fwd(...,
           out="bf16") unchanged; dt_layernorm adds 16 values per lane, then a 4-step butterfly: depth 20,
           within ln_cases.depth(256) = 64.
A check returns error / tolerance per row (the maximum over the row's elements; lse: per object, head,
query); nothing is scaled by a whole-tensor maximum.

model32() is an fp32 model of the kernels' own arithmetic: bf16 rounding exactly where the header of
decoder_tok.hip lists it (each projection output, each add, each LayerNorm output, P for P V), sequential
fp32 sums over k, softmax as the kernel (max, exp2, P rounded, inv = 1 / l), LayerNorm lanes as dt_layernorm
(lane j takes columns j + 16 i), with the switchable DEFECTS.  test_decoder_tok_host.py proves that the
clean model holds every assertion with a factor 4 to spare on the value before the output rounding (<= 1 on
the rounded one, equality where claimed) and that each defect breaks the assertion DEFECT_SITES names by
more than 10x.

The constants were set from the clean model against float64, never from the kernels: each the smallest of
1, 2, 3, 4 that keeps the clean model's worst ratio, before the output rounding, under a quarter over all
shapes, classes and flags (test_decoder_tok_host.py::test_clean_model_within_quarter prints them with -s):
  proj  0.070  dt_self T 8 x 3 ln, qs        (C_PROJ 1)
  lse   0.091  dt_self T 8 x 13 softmax      (C_LSE 1)
  os    0.240  dt_self T 3 x 6 softmax       (C_OS 1, with the corrected formula below)
  LayerNorm, with ln_cases' own constants: y 0.188, rstd 0.213, mean < 0.001 (sums of 16 bf16 values of one
  binade are exact in fp32)
For os "before the output rounding" also means before the rounding of P (the 2^-8 terms are dropped together
and the model's unrounded P is used): with P rounded the clean model reaches 0.79 of the full tolerance, as a
rounded output reaches 0.99 of rnd(v), by construction.

Two corrections of the os formula as first written (rnd(os) + 2^-8 sum p |v| + C_OS (delta_i sum_j p_ij
|v_jc - o_ic| + T u sum_j p_ij |v_jc|)), both because the clean model broke it, neither by widening a constant:
  * (3 T + 4) u instead of T u.  With one dominant key (p ~ 1) at T = 3 the clean model is off by 3.1 u |o|,
    1.04 of a term that counts only the T additions of P V; the chain really has, per key, a product, an
    addition and an addition into the normaliser (3 T), then exp2 (1 ulp = 2 u), 1 / l and the final product.
    With T u no constant up to 4 keeps the quarter.
  * 2^-126 sum_j |v_jc|: an unnormalised probability below the smallest normal fp32 / bf16 number may be
    flushed to zero.  In the exact class the scores are hundreds of nats apart and the float64 reference
    keeps contributions of 1e-60 that no fp32 softmax can hold; where the dominant key's v is 0 they are
    the whole reference value and the relative terms vanish."""
import collections
import functools
import math
import zlib

import numpy as np

import ln_cases as lc

U = lc.U
F32, F64 = np.float32, np.float64
SENT = -9.0           # as gemm_exact_cases.SENT: fills every output element no launch may write
C, CI, HEADS, HD = 256, 128, 8, 32
ROWS_PER_WG = 16
SHAPES = [(8, 1), (8, 2), (8, 3),
          (8, 13),    # the workload's own 104 rows
          (7, 3),     # two dead LDS rows per workgroup, then a partial workgroup
          (5, 4),     # three objects (15 rows), then one object
          (3, 6),
          (1, 17),    # 16 single-token objects, then one; softmax over one key
          (9, 2),     # one object per workgroup, seven dead rows
          (16, 2)]    # full tile
KERNELS = ("self", "post_a", "post_b", "final")
EPS = lc.EPS
C_PROJ, C_LSE, C_OS = 1.0, 1.0, 1.0
TINY = 2.0 ** -126    # an unnormalised probability below it may be flushed to zero (fp32, and bf16 for P V)

Case = collections.namedtuple("Case", "kernel T objects cls flag eps")

# slot -> (source, residual or None); "qin" is qa, or x when skip
PROJ = {"qs": ("qin", None), "ks": ("qin", None), "vs": ("x", None), "y1": ("os", "x unless skip"), "qq": ("qt", None),
        "y2": ("ot", "x1"), "kio": ("q2", None), "vio": ("x3", None), "qqf": ("qfa", None), "y": ("of", "x3")}
EQUAL_SLOTS = {"self": ("qs", "ks", "vs"), "post_a": ("y2",), "post_b": (), "final": ("y",)}
ADD_SLOTS = ("qa", "qt", "q2", "qfa")

# kernel -> [(slot, kind)], kind: 256 / 128 = bf16 [R, width]; "stat" = fp32 [R]; "lse" = fp32 [objects, 8, T]
OUTPUTS = {
    "self": [("qa", 256), ("qs", 256), ("ks", 256), ("vs", 256), ("os", 256), ("lse", "lse"), ("y1", 256), ("x1", 256),
             ("mean1", "stat"), ("rstd1", "stat"), ("qt", 256), ("qq", 128)],
    "post_a": [("y2", 256), ("x2", 256), ("mean2", "stat"), ("rstd2", "stat")],
    "post_b": [("x3", 256), ("mean3", "stat"), ("rstd3", "stat"), ("q2", 256), ("kio", 128), ("vio", 128), ("qfa", 256),
               ("qqf", 128)],
    "final": [("y", 256), ("hs", 256), ("mean", "stat"), ("rstd", "stat")],
}

DEFECTS = {
    "v_from_qa": "the v projection fed from x + pe instead of x",
    "skip_adds_pe": "skip = 1 still projects q / k from x + pe",
    "skip_keeps_residual": "skip = 1 still adds x to the out-projection",
    "residual_dropped": "an out-projection without its residual",
    "no_max_subtract": "softmax as exp2(s) / sum exp2(s)",
    "scale_missing": "scores not multiplied by scale",
    "lse_base2": "lse left in log2 units",
    "neighbour_object_keys": "softmax keys taken from the next object of the workgroup",
    "head_offset_wrong": "keys read at the next head's channels",
    "ki_from_x3": "the image -> token key projection fed from x3 instead of x3 + pe",
    "vi_from_q2": "the image -> token value projection fed from x3 + pe instead of x3",
    "qq_from_x1": "the token -> image query projection fed from x1 instead of x1 + pe",
    "bias_column_shift": "bias[col + 1] added to column col",
    "ln_one_pass": "variance as E[x^2] - mu^2",
    "ln_eps_outside": "rs = 1 / (sqrt(var) + eps)",
    "ln_stats_before_round": "mean / rstd of the projection output before its bf16 rounding",
}
def _eps(T, O, flag):
    """the eps of a case outside the ln / bias300 classes (those run both)"""
    return EPS[(T + O + flag) % 2]


def find(kernel, T, O, cls, flag):
    """the case of a class that runs one eps per shape and flag"""
    return Case(kernel, T, O, cls, flag, _eps(T, O, flag))


# defect -> (the case, the assertion it must break by more than 10x; an equality assertion: break it)
DEFECT_SITES = {
    "v_from_qa": (find("self", 8, 2, "real", 0), "vs"),
    "skip_adds_pe": (find("self", 8, 2, "real", 1), "qs"),
    "skip_keeps_residual": (find("self", 8, 2, "real", 1), "y1"),
    "residual_dropped": (find("post_a", 7, 3, "real", 0), "y2"),
    "no_max_subtract": (find("self", 5, 4, "softmax", 0), "os"),
    "scale_missing": (find("self", 5, 4, "softmax", 0), "lse"),
    "lse_base2": (find("self", 5, 4, "softmax", 1), "lse"),
    "neighbour_object_keys": (find("self", 8, 2, "softmax", 0), "os"),
    "head_offset_wrong": (find("self", 3, 6, "softmax", 0), "os"),
    "ki_from_x3": (find("post_b", 5, 4, "real", 0), "kio"),
    "vi_from_q2": (find("post_b", 5, 4, "real", 1), "vio"),
    "qq_from_x1": (find("self", 9, 2, "real", 0), "qq"),
    "bias_column_shift": (find("self", 8, 3, "exact", 0), "qs"),
    "ln_one_pass": (Case("post_b", 8, 13, "ln", 0, 1e-6), "rstd3"),
    "ln_eps_outside": (Case("post_a", 8, 13, "ln", 0, 1e-5), "rstd2"),
    "ln_stats_before_round": (Case("final", 7, 3, "bias300", 0, 1e-6), "mean"),
}


def cases(kernel):
    """every (shape, class, flag, eps) of one kernel; flag is skip (dt_self), final_q (dt_post_b), else 0"""
    flags = (0, 1) if kernel in ("self", "post_b") else (0,)
    out = []
    for T, O in SHAPES:
        for flag in flags:
            for cls in ("exact", "real") + (("softmax",) if kernel == "self" else ()):
                out.append(find(kernel, T, O, cls, flag))
            for eps in EPS:
                out.append(Case(kernel, T, O, "ln", flag, eps))
    for T, O in ((8, 13), (7, 3)):
        for flag in flags:
            for eps in EPS:
                out.append(Case(kernel, T, O, "bias300", flag, eps))
    return out


def case_id(c):
    return f"{c.kernel} T{c.T}x{c.objects} {c.cls} flag{c.flag} eps{c.eps:g}"


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _ro(a):
    a.setflags(write=False)
    return a


round_bf16 = lc.round_bf16


def _bf(a):
    return round_bf16(np.asarray(a, F32))


# ------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def _weight(name, N, K, kind):
    """(W [N, K] bf16 values, b [N] fp32); kind: tern / real / zero / bias300"""
    g = _rng("w", name, N, K, kind)
    if kind == "tern":
        return _ro(g.integers(-1, 2, (N, K)).astype(F32)), _ro(g.integers(-3, 4, N).astype(F32))
    if kind == "zero":
        return _ro(np.zeros((N, K), F32)), _ro(np.zeros(N, F32))
    w = _bf(g.standard_normal((N, K)) / math.sqrt(K))
    b = (0.1 * g.standard_normal(N)).astype(F32)
    if kind == "bias300":
        b = (300 + b).astype(F32)
    return _ro(w), _ro(b)


def _act(name, c, width, kind):
    g = _rng("a", name, c.T, c.objects, c.flag, width, kind)
    R = c.T * c.objects
    if kind == "tern":
        return _ro(g.integers(-1, 2, (R, width)).astype(F32))
    return _ro(_bf(g.standard_normal((R, width))))


def _ln_rows(c):
    """R rows of ln_cases.make_rows(256, "bf16"), starting at a row that moves with the shape, so that the
    small shapes together see every regime too"""
    rows, names = lc.make_rows(C, "bf16")
    R = c.T * c.objects
    idx = (np.arange(R) + 3 * c.T + c.objects) % rows.shape[0]
    return _ro(rows[idx].copy()), tuple(names[i] for i in idx)


STEP = 2.0 ** -4
GAINS = [0.0, 1.0, 2.5, 3.9, 4.0, 6.3, -4.0, -6.3]   # as attn_cases.GAINS
SPIKE = 11.0
SM_REGIMES = ("flat", "peaked", "shift+60", "shift-60")


def _snap(v):
    return np.round(np.asarray(v, F64) / STEP) * STEP


def sm_regime(o, h):
    return SM_REGIMES[(o + h) % 4]


def _softmax_qin(c):
    """the [R, 256] tensor q and k are selected from (x + pe, or x when skip): q of steered head h at
    channels 32 h .., its k at 128 + 32 h .."""
    g = _rng("softmax", c.T, c.objects, c.flag)
    T, O = c.T, c.objects
    gq = HD ** -0.25
    t = np.zeros((O, T, C), F64)
    alt = np.ones(HD)
    alt[1::2] = -1
    for o in range(O):
        for h in range(4):
            su = g.integers(0, 2, HD) * 2.0 - 1
            sw = su * alt

            def noise():
                e = _snap(np.clip(0.3 * g.standard_normal((T, HD // 2)), -0.9, 0.9))
                n = np.empty((T, HD))
                n[:, 0::2] = e
                n[:, 1::2] = e * su[0::2] * su[1::2]   # orthogonal to sw
                return n
            reg = sm_regime(o, h)
            a = np.array([GAINS[i % 8] for i in range(T)])
            nq, nk = noise(), noise()
            if reg == "flat":
                q = nq + _snap(a * gq)[:, None] * su
                k = np.broadcast_to(_snap(2.5 * gq) * su, (T, HD))
            elif reg == "peaked":
                cj = np.zeros(T)
                cj[o % T] = SPIKE
                q = nq + _snap(SPIKE * gq) * su
                k = nk + _snap(cj * gq)[:, None] * su
            else:
                sgn = 1.0 if reg == "shift+60" else -1.0
                rho = _snap(math.sqrt(60.0) * gq)
                cj = 6.3 * np.arange(T) / max(T - 1, 1)
                q = nq + _snap(a * gq)[:, None] * su + rho * sw
                k = nk + _snap(cj * gq)[:, None] * su + sgn * rho * sw
            t[o, :, HD * h:HD * (h + 1)] = q
            t[o, :, CI + HD * h:CI + HD * (h + 1)] = k
            if reg == "peaked" and T > 1:
                s = (q @ k.T) * HD ** -0.5
                gap = s[:, o % T] - np.delete(s, o % T, axis=1).max(axis=1)
                assert gap.min() >= 100, (c, o, h, gap.min())
    assert np.abs(t).max() < 7
    return t.reshape(O * T, C)


@functools.lru_cache(maxsize=None)
def _select_weights():
    """Wq / Wk of the softmax class: rows 0..127 select channel n (q) / 128 + n (k), rows 128..255 dense"""
    wq, bq = (a.copy() for a in _weight("wq", C, C, "real"))
    wk, bk = (a.copy() for a in _weight("wk", C, C, "real"))
    wq[:CI], wk[:CI], bq[:CI], bk[:CI] = 0, 0, 0, 0
    wq[np.arange(CI), np.arange(CI)] = 1
    wk[np.arange(CI), CI + np.arange(CI)] = 1
    return _ro(wq), _ro(bq), _ro(wk), _ro(bk)


@functools.lru_cache(maxsize=None)
def build(c):
    """the inputs of case c: {name: fp32 array holding bf16 values (activations, weights) or fp32 values
    (biases, gamma, beta)} + "scale" / "eps".  Shared: do not write into them."""
    k = c.kernel
    kind = "tern" if c.cls == "exact" else "real"
    gamma, beta = lc.make_params(C, seed={"self": 1, "post_a": 2, "post_b": 3, "final": 4}[k])
    inp = {"eps": lc.f32(c.eps)}
    # the projection in front of the LayerNorm
    okind = {"ln": "zero", "bias300": "bias300"}.get(c.cls, kind)
    if k == "self":
        inp["scale"] = lc.f32(HD ** -0.5)
        inp["x"], inp["pe"] = _act("x", c, C, kind), _act("pe", c, C, kind)
        for n in ("q", "k", "v"):
            inp["w" + n], inp["b" + n] = _weight("w" + n, C, C, kind)
        inp["wo"], inp["bo"] = _weight("wo", C, C, okind)
        inp["wqc"], inp["bqc"] = _weight("wqc", CI, C, kind)
        inp["g1"], inp["b1"] = gamma, beta
        if c.cls == "ln":
            inp["x"], inp["ln_names"] = _ln_rows(c)
        if c.cls == "softmax":
            inp["wq"], inp["bq"], inp["wk"], inp["bk"] = _select_weights()
            t = _softmax_qin(c)
            pe = _snap(np.clip(_rng("sm-pe", c.T, c.objects).standard_normal(t.shape), -1, 1))
            x = t if c.flag else t - pe
            inp["x"], inp["pe"] = _ro(x.astype(F32)), _ro(pe.astype(F32))
            for a in (inp["x"], inp["pe"]):
                assert np.array_equal(_bf(a), a) and np.array_equal(a.astype(F64) / STEP, np.round(a / STEP))
    elif k == "post_a":
        inp["ot"], inp["x1"] = _act("ot", c, CI, kind), _act("x1", c, C, kind)
        inp["wo"], inp["bo"] = _weight("wo_a", C, CI, okind)
        inp["g2"], inp["b2"] = gamma, beta
        if c.cls == "ln":
            inp["x1"], inp["ln_names"] = _ln_rows(c)
    elif k == "post_b":
        inp["y3"], inp["pe"] = _act("y3", c, C, kind), _act("pe_b", c, C, kind)
        for n in ("ki", "vi", "qf"):
            inp["w" + n], inp["b" + n] = _weight("w" + n, CI, C, kind)
        inp["g3"], inp["b3"] = gamma, beta
        if c.cls == "ln":
            inp["y3"], inp["ln_names"] = _ln_rows(c)
        if c.cls == "bias300":
            inp["y3"] = _ro(_bf(300 + inp["y3"]))
    else:
        inp["of"], inp["x3"] = _act("of", c, CI, kind), _act("x3", c, C, kind)
        inp["wo"], inp["bo"] = _weight("wo_f", C, CI, okind)
        inp["g"], inp["b"] = gamma, beta
        if c.cls == "ln":
            inp["x3"], inp["ln_names"] = _ln_rows(c)
    if c.cls == "exact":
        for slot in EQUAL_SLOTS[k]:
            for a, w in _exact_products(c, inp, slot):
                assert np.abs(a.astype(F64) @ w.astype(F64).T).max() <= 256, (c, slot)
    return inp


def _exact_products(c, inp, slot):
    if c.kernel == "self":
        src = inp["x"] if (slot == "vs" or c.flag) else inp["x"] + inp["pe"]
        return [(src, inp["w" + slot[0]])]
    return [(inp["ot" if c.kernel == "post_a" else "of"], inp["wo"])]


def present(c):
    """the output slots case c writes: qa only without skip, qfa / qqf only with final_q"""
    skip = set()
    if c.kernel == "self" and c.flag:
        skip = {"qa"}
    if c.kernel == "post_b" and not c.flag:
        skip = {"qfa", "qqf"}
    return [(n, kind) for n, kind in OUTPUTS[c.kernel] if n not in skip]


def slot_shape(c, kind):
    R = c.T * c.objects
    return (R,) if kind == "stat" else (c.objects, HEADS, c.T) if kind == "lse" else (R, kind)


# ------------------------------------------------------------------ fp32 model of the kernels' arithmetic
def _lin32(a, w, b, res=None, defects=()):
    """fp32 acc over k in order, + bias (+ residual): the value before the store's rounding"""
    a, wt = np.asarray(a, F32), np.ascontiguousarray(np.asarray(w, F32).T)
    acc = np.zeros((a.shape[0], wt.shape[1]), F32)
    for k in range(wt.shape[0]):
        acc = acc + a[:, k:k + 1] * wt[k]
    b = np.asarray(b, F32)
    v = acc + (np.roll(b, -1) if "bias_column_shift" in defects else b)
    if res is not None and "residual_dropped" not in defects:
        v = v + np.asarray(res, F32)
    return v.astype(F32)


def _ln32(raw, y, gamma, beta, eps, defects=()):
    """dt_layernorm on y = bf16(raw): 16 lanes per row, lane j sums columns j + 16 i in order, then a xor
    butterfly -> (x fp32 before the store's rounding, mean, rstd)"""
    d = [n[3:] for n in defects if n in ("ln_one_pass", "ln_eps_outside")]
    src = raw if "ln_stats_before_round" in defects else y
    _, mu, rs, _ = lc.fwd32(src, gamma, beta, eps, 16, 16, 1, defects=d)
    x = (y - mu[:, None]) * rs[:, None] * np.asarray(gamma, F32) + np.asarray(beta, F32)
    return x.astype(F32), mu, rs


def _attn32(c, q, k, v, scale, defects=()):
    """dt_self's attention -> (os fp32 before the store's rounding [R, 256], lse [objects, 8, T])"""
    T, O = c.T, c.objects
    q, k, v = (np.asarray(t, F32).reshape(O, T, HEADS, HD) for t in (q, k, v))
    if "head_offset_wrong" in defects:
        k = np.roll(k, -1, axis=2)
    if "neighbour_object_keys" in defects:
        per = ROWS_PER_WG // T
        nb = [(o // per) * per + (o % per + 1) % min(per, O - (o // per) * per) for o in range(O)]
        k = k[nb]
    sl2 = F32(1 if "scale_missing" in defects else scale) * F32(1.4426950408889634)
    d = np.zeros((O, HEADS, T, T), F32)
    for ch in range(HD):
        d = d + q[:, :, :, ch].transpose(0, 2, 1)[:, :, :, None] * k[:, :, :, ch].transpose(0, 2, 1)[:, :, None, :]
    s = (d * sl2).astype(F32)
    mx = s.max(axis=3)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        e = np.exp2(s if "no_max_subtract" in defects else s - mx[..., None]).astype(F32)
        l = np.zeros((O, HEADS, T), F32)
        for j in range(T):
            l = l + e[..., j]
        pb = round_bf16(np.where(np.isfinite(e), e, 0)).astype(F32)
        pb = np.where(np.isfinite(e), pb, e)
        inv = F32(1) / l
        acc, acc_e = np.zeros((O, HEADS, T, HD), F32), np.zeros((O, HEADS, T, HD), F32)
        for j in range(T):
            acc = acc + pb[..., j][..., None] * v[:, j][:, :, None, :]
            acc_e = acc_e + e[..., j][..., None] * v[:, j][:, :, None, :]
        o = (acc * inv[..., None]).astype(F32)
        o_e = (acc_e * inv[..., None]).astype(F32)   # without the rounding of P: for the quarter margin
        lg = np.log2(l).astype(F32)
        lse = lg if "no_max_subtract" in defects else (mx + lg).astype(F32)
        if "lse_base2" not in defects:
            lse = (lse * F32(0.6931471805599453)).astype(F32)
    return o.transpose(0, 2, 1, 3).reshape(O * T, C), o_e.transpose(0, 2, 1, 3).reshape(O * T, C), lse


def model32(c, inp, defects=()):
    """(out, raw): every output slot as the kernel stores it (bf16 values / fp32), and the fp32 value before
    the store's rounding of every bf16 slot"""
    out, raw = {}, {}
    eps = inp["eps"]

    def put(name, v):
        raw[name] = np.asarray(v, F32)
        out[name] = round_bf16(raw[name])
        return out[name]

    def ln(src, names, g, b):
        x, mu, rs = _ln32(raw[src], out[src], g, b, eps, defects)
        out[names[1]], out[names[2]] = mu, rs
        return put(names[0], x)
    k = c.kernel
    if k == "self":
        x, pe, skip = inp["x"], inp["pe"], c.flag
        qa = round_bf16(x + pe)
        if not skip:
            put("qa", x + pe)
        qin = qa if (not skip or "skip_adds_pe" in defects) else x
        q = put("qs", _lin32(qin, inp["wq"], inp["bq"], defects=defects))
        kk = put("ks", _lin32(qin, inp["wk"], inp["bk"], defects=defects))
        v = put("vs", _lin32(qa if "v_from_qa" in defects else x, inp["wv"], inp["bv"], defects=defects))
        o, o_e, out["lse"] = _attn32(c, q, kk, v, inp["scale"], defects)
        o = put("os", o)
        raw["os"] = o_e
        res = x if (not skip or "skip_keeps_residual" in defects) else None
        put("y1", _lin32(o, inp["wo"], inp["bo"], res, defects))
        x1 = ln("y1", ("x1", "mean1", "rstd1"), inp["g1"], inp["b1"])
        qt = put("qt", x1 + pe)
        put("qq", _lin32(x1 if "qq_from_x1" in defects else qt, inp["wqc"], inp["bqc"], defects=defects))
    elif k == "post_a":
        put("y2", _lin32(inp["ot"], inp["wo"], inp["bo"], inp["x1"], defects))
        ln("y2", ("x2", "mean2", "rstd2"), inp["g2"], inp["b2"])
    elif k == "post_b":
        raw["y3"] = out["y3"] = inp["y3"]
        x3 = ln("y3", ("x3", "mean3", "rstd3"), inp["g3"], inp["b3"])
        del raw["y3"], out["y3"]
        q2 = put("q2", x3 + inp["pe"])
        put("kio", _lin32(x3 if "ki_from_x3" in defects else q2, inp["wki"], inp["bki"], defects=defects))
        put("vio", _lin32(q2 if "vi_from_q2" in defects else x3, inp["wvi"], inp["bvi"], defects=defects))
        if c.flag:
            put("qfa", x3 + inp["pe"])
            put("qqf", _lin32(out["qfa"], inp["wqf"], inp["bqf"], defects=defects))
    else:
        put("y", _lin32(inp["of"], inp["wo"], inp["bo"], inp["x3"], defects))
        ln("y", ("hs", "mean", "rstd"), inp["g"], inp["b"])
    return out, raw


# ------------------------------------------------------------------ float64 stage checks
_ratio = lc._ratio


def _rows(r):
    """the maximum over everything but the first axis; NaN (a NaN output) counts as infinite"""
    r = np.where(np.isnan(r), np.inf, r)
    return r.reshape(r.shape[0], -1).max(axis=1)


def check_equal(got, want):
    """ratio 0 where equal, inf where not (NaN never equal)"""
    return _rows(np.where(np.asarray(got) == np.asarray(want), 0.0, np.inf))


def check_add(got, a, b):
    return check_equal(got, round_bf16(np.asarray(a, F32) + np.asarray(b, F32)))


def check_proj(got, a, w, b, res=None, out="bf16"):
    """got [R, N] against a W^T + b (+ res) in float64; out: "bf16" (stored) or None (before the rounding)"""
    a, w, b = np.asarray(a, F64), np.asarray(w, F64), np.asarray(b, F64)
    ref = a @ w.T + b
    mag = np.abs(a) @ np.abs(w).T + np.abs(b)
    if res is not None:
        ref, mag = ref + np.asarray(res, F64), mag + np.abs(np.asarray(res, F64))
    tol = (2.0 ** -8 * np.abs(ref) if out == "bf16" else 0.0) + C_PROJ * a.shape[1] * U * mag
    return _rows(_ratio(np.abs(np.asarray(got, F64) - ref), tol))


def attn64(c, q, k, v, scale):
    T, O = c.T, c.objects
    q, k, v = (np.asarray(t, F64).reshape(O, T, HEADS, HD).transpose(0, 2, 1, 3) for t in (q, k, v))  # [O, H, T, D]
    s = scale * np.einsum("ohic,ohjc->ohij", q, k)
    sabs = scale * np.einsum("ohic,ohjc->ohij", np.abs(q), np.abs(k)).max(axis=3)
    mx = s.max(axis=3, keepdims=True)
    e = np.exp(s - mx)
    l = e.sum(axis=3, keepdims=True)
    p = e / l
    lse = (mx + np.log(l))[..., 0]
    o = np.einsum("ohij,ohjc->ohic", p, v)
    pv = np.einsum("ohij,ohjc->ohic", p, np.abs(v))
    dev = np.einsum("ohij,ohijc->ohic", p, np.abs(v[:, :, None, :, :] - o[:, :, :, None, :]))
    vsum = np.broadcast_to(np.abs(v).sum(axis=2, keepdims=True), o.shape)
    return dict(o=o, lse=lse, pv=pv, dev=dev, delta=32 * U * sabs, p=p, vsum=vsum)


def check_attn(c, os_, lse, q, k, v, scale, out="bf16"):
    """-> {"os": ratio per row, "lse": ratio per (object, head, query) flattened}"""
    T, O = c.T, c.objects
    r = attn64(c, q, k, v, float(scale))
    got = np.asarray(os_, F64).reshape(O, T, HEADS, HD).transpose(0, 2, 1, 3)
    rounding = 2.0 ** -8 * (np.abs(r["o"]) + r["pv"]) if out == "bf16" else 0.0   # of the output and of P
    tol = rounding + TINY * r["vsum"] + C_OS * (r["delta"][..., None] * r["dev"] + (3 * T + 4) * U * r["pv"])
    ro = _ratio(np.abs(got - r["o"]), tol)
    ro = np.where(np.isnan(ro), np.inf, ro).max(axis=3).transpose(0, 2, 1).max(axis=2).reshape(O * T)  # per row
    tl = C_LSE * (r["delta"] + U * (np.abs(r["lse"]) + 4))
    rl = _ratio(np.abs(np.asarray(lse, F64).reshape(O, HEADS, T) - r["lse"]), tl)
    return {"os": ro, "lse": np.where(np.isnan(rl), np.inf, rl).reshape(-1)}


def check(c, inp, out, raw=None):
    """every assertion of case c -> {slot: ratio per row}.  out: the stored slots (fp32 arrays of bf16 / fp32
    values); the stage inputs are always taken from it.  raw: check instead the fp32 values before the
    store's rounding against the tolerance without the output rounding (the quarter margin)."""
    val = (lambda n: raw[n]) if raw is not None else (lambda n: out[n])
    ot = None if raw is not None else "bf16"
    res, eps, k = {}, inp["eps"], c.kernel
    exact = c.cls == "exact"

    def proj(slot, a, w, b, r=None):
        res[slot] = check_proj(val(slot), a, inp[w], inp[b], r, ot)
        if exact and raw is None and slot in EQUAL_SLOTS[k]:
            ref = np.asarray(a, F64) @ inp[w].astype(F64).T + inp[b] + (0 if r is None else r)
            res[slot] = np.maximum(res[slot], check_equal(out[slot], ref))

    def ln(src, names, g, b):
        r = lc.check_fwd(src, inp[g], inp[b], eps, y=val(names[0]), mean=out[names[1]], rstd=out[names[2]], out=ot)
        res[names[0]], res[names[1]], res[names[2]] = (np.where(np.isnan(r[n]), np.inf, r[n]) for n in ("y", "mean", "rstd"))

    def add(slot, a, b):
        if raw is None:
            res[slot] = check_add(out[slot], a, b)
    if k == "self":
        x, pe = inp["x"], inp["pe"]
        if not c.flag:
            add("qa", x, pe)
        qin = x if c.flag else out["qa"]
        proj("qs", qin, "wq", "bq")
        proj("ks", qin, "wk", "bk")
        proj("vs", x, "wv", "bv")
        res.update(check_attn(c, val("os"), out["lse"], out["qs"], out["ks"], out["vs"], inp["scale"], ot))
        proj("y1", out["os"], "wo", "bo", None if c.flag else x)
        ln(out["y1"], ("x1", "mean1", "rstd1"), "g1", "b1")
        add("qt", out["x1"], pe)
        proj("qq", out["qt"], "wqc", "bqc")
    elif k == "post_a":
        proj("y2", inp["ot"], "wo", "bo", inp["x1"])
        ln(out["y2"], ("x2", "mean2", "rstd2"), "g2", "b2")
    elif k == "post_b":
        ln(inp["y3"], ("x3", "mean3", "rstd3"), "g3", "b3")
        add("q2", out["x3"], inp["pe"])
        proj("kio", out["q2"], "wki", "bki")
        proj("vio", out["x3"], "wvi", "bvi")
        if c.flag:
            add("qfa", out["x3"], inp["pe"])
            proj("qqf", out["qfa"], "wqf", "bqf")
    else:
        proj("y", inp["of"], "wo", "bo", inp["x3"])
        ln(out["y"], ("hs", "mean", "rstd"), "g", "b")
    return res


def worst(res):
    """{slot: (max ratio, row)}"""
    return {n: (float(r.max()), int(r.argmax())) for n, r in res.items()}


# ------------------------------------------------------------------ guarded buffers
class Arena:
    """Slots of one element type inside a flat buffer of `fill`: before and after each slot a guard of 16, 24
    or 32 elements (a multiple of 8, so every base stays 16-byte aligned), and after its payload `tail`
    more elements of fill (the rows past R of an output)."""

    def __init__(self, fill):
        self.fill, self.n, self.slots = fill, 16, {}

    def add(self, name, shape, tail=0):
        size = int(np.prod(shape))
        assert self.n % 8 == 0
        self.slots[name] = (self.n, tuple(shape))
        self.n += (size + tail + 7) // 8 * 8 + (16, 24, 32)[len(self.slots) % 3]

    def host(self, values=None):
        """the flat fp32 array: fill everywhere, values[name] in its slot"""
        a = np.full(self.n, self.fill, F32)
        for name, (off, shape) in self.slots.items():
            if values is not None:
                a[off:off + int(np.prod(shape))] = np.asarray(values[name], F32).reshape(-1)
        return a

    def offset(self, name):
        return self.slots[name][0]

    def read(self, flat):
        """flat (as host()) -> ({name: array}, ok): ok is False when an element outside the slots changed"""
        mask = np.zeros(self.n, bool)
        got = {}
        for name, (off, shape) in self.slots.items():
            size = int(np.prod(shape))
            mask[off:off + size] = True
            got[name] = flat[off:off + size].reshape(shape).copy()
        return got, bool((flat[~mask] == self.fill).all())
