"""ln_cases.py can fail, and only where it should (no GPU): the float64 models are torch's float64
layer_norm and its autograd; the clean fp32 model of the kernels' arithmetic stays within a quarter of every
tolerance at every (regime, C, eps, type, lane layout); every switchable defect of that model breaks a named
assertion by more than 10x on named regimes at every size it applies to; and the randn rows that the older
LayerNorm tests draw do not see the statistics defects.

What the last point proves, exactly.  Under the older tests' own check (test_kernels_gpu.py _close: the
maximum error of the tensor against 1e-5 (fp32) / 1e-2 (bf16) of the tensor's maximum, eps 1e-6) randn
rows pass a one-pass variance, an eps outside the square root and statistics taken before the bf16 rounding
in both types.  Division by C - 1 passes in bf16 only: it scales y by 1 + 1 / 2C, which the fp32 tolerance
of 1e-5 does see on any rows.  The same four defects on the rows of ln_cases.py fail that very check or
the per-row ones by orders of magnitude (test_defect_breaks_a_named_assertion)."""
import numpy as np
import pytest
import torch

import ln_cases as L

F64 = np.float64

# defect -> (assertions that must break, regimes that break them, applies(dtype, C, G, K, VEC))
CATCH = {
    # (bf16 at C = 8: the squares, 16 significant bits, and their sum are exact in fp32 -- no defect to see)
    "one_pass": (("rstd", "y"), ("offset300", "offset30", "const_ulp", "neg_offset"),
                 lambda d, C, G, K, V: not (d == "bf16" and C <= 8)),
    "eps_outside": (("rstd", "y"), ("const", "zero", "tiny", "const_ulp"), None),
    "bessel": (("rstd", "y"), ("randn", "outlier", "large"), None),
    "stats_before_round": (("mean", "rstd", "y"), ("offset300", "neg_offset"), lambda d, C, G, K, V: d == "bf16"),
    "padded_count": (("mean", "rstd", "y"), ("offset300", "offset30", "const", "neg_offset"),
                     lambda d, C, G, K, V: G * K * V != C),
    "mean_dead_lane": (("mean", "rstd", "y"), ("offset300", "offset30", "const", "neg_offset"), None),
    "bwd_s2_no_gamma": (("dx",), ("randn", "outlier", "large"), None),
    "bwd_means_no_rstd": (("dx",), ("const", "zero", "tiny", "const_ulp", "offset30"), None),
    "dgamma_x": (("dgamma",), None, None),
    "bwd_addend_dropped": (("dx",), ("randn", "offset300", "large"), None),
}
STAT_DEFECTS = ["one_pass", "eps_outside", "bessel", "stats_before_round"]
SIZE_IDS = [f"{d}-{C}" for d, C in L.SIZES]


def _layouts(dtype, C):
    """the vector plan's lane layout (where there is one) and the scalar kernels'"""
    out = [L.lanes(C, dtype, scalar=True)]
    if L.plan(C, dtype)[0] == "vec":
        out.insert(0, L.lanes(C, dtype))
    return out


def _run(dtype, C, eps, G, K, V, defects=(), store=True):
    """every assertion of ln_cases on the fp32 model: plain forward, forward with the rounding pre-add,
    backward with dres into non-zero dgamma / dbeta -> ({name: ratio per row / column}, regime names)"""
    x, names = L.make_rows(C, dtype)
    gamma, beta = L.make_params(C)
    dy = L.make_noise(L.NROWS, C, dtype, 1)
    dres = L.make_noise(L.NROWS, C, dtype, 2)
    dg0, db0 = L.make_noise(2, C, "fp32", 3)
    out = dtype if store else None
    rnd = (lambda v: L.round_to(v, dtype)) if store else (lambda v: v)
    res = {}

    def merge(r):
        for k, v in r.items():
            res[k] = np.maximum(res[k], v) if k in res else v

    y, mu, rs, _ = L.fwd32(x, gamma, beta, eps, G, K, V, defects)
    merge(L.check_fwd(x, gamma, beta, eps, rnd(y), mu, rs, out=out))
    for bcast in (False, True):
        add = L.rounding_addend(x, dtype, bcast)
        y2, mu2, rs2, xs = L.fwd32(x, gamma, beta, eps, G, K, V, defects, add=add, dtype=dtype)
        assert np.array_equal(xs, L.preadd(x, add, dtype))
        merge(L.check_fwd(xs, gamma, beta, eps, rnd(y2), mu2, rs2, out=out))
    # the backward reads the statistics a *clean* forward saved: its defects are its own
    _, mu, rs, _ = L.fwd32(x, gamma, beta, eps, G, K, V)
    dx, dg, db = L.bwd32(x, dy, gamma, mu, rs, G, K, V, defects, addend=dres, dg0=dg0, db0=db0)
    merge(L.check_bwd(x, dy, gamma, eps, rnd(dx), dg, db, addend=dres, dg0=dg0, db0=db0, out=out))
    return res, names


# ------------------------------------------------------------------ the inputs are what they claim
@pytest.mark.parametrize("dtype,C", L.SIZES, ids=SIZE_IDS)
def test_rows_are_storage_values_and_ragged(dtype, C):
    x, names = L.make_rows(C, dtype)
    assert x.shape == (70, C) and sorted(set(names)) == sorted(L.REGIMES)
    assert np.array_equal(L.round_to(x, dtype), x)
    for G in (1, 2, 4, 8, 16, 32, 64):
        assert 70 % (4 * (64 // G)) != 0  # a ragged last block at every rows-per-block
    i = names.index("const_ulp")
    assert np.sum(x[i] != L.CONST) == 1 and x[i].max() == L.CONST + 2.0 ** -6
    if dtype == "bf16":
        for bcast in (False, True):
            add = L.rounding_addend(x, dtype, bcast)
            exact = x.astype(F64) + add.astype(F64)
            off = [r for r, n in enumerate(names) if n in ("offset300", "neg_offset")]
            inexact = (L.preadd(x, add, dtype).astype(F64) != exact)[off]
            assert inexact.mean() > 0.9, "a + b must really round on the offset rows"


def test_plan_rule_gives_the_dispatch_table():
    """norm.hip plan() as ln_cases.plan() recomputes it: the <G, K> of every size the GPU file runs"""
    want = {("bf16", 8): (1, 1), ("bf16", 16): (2, 1), ("bf16", 32): (4, 1), ("bf16", 64): (8, 1), ("bf16", 112): (16, 1),
            ("bf16", 256): (32, 1), ("bf16", 512): (64, 1), ("bf16", 896): (64, 2), ("bf16", 1280): (64, 3),
            ("fp32", 4): (1, 1), ("fp32", 112): (32, 1), ("fp32", 256): (64, 1), ("fp32", 448): (64, 2),
            ("fp32", 896): (64, 5), ("fp32", 1280): (64, 5)}
    for (dtype, C), (G, K) in want.items():
        assert L.plan(C, dtype, (C, C), (4096, 8192)) == ("vec", G, K), (dtype, C)
    # all ten <G, K> instantiations of S2H_LN_DISPATCH
    assert set(want.values()) == {(1, 1), (2, 1), (4, 1), (8, 1), (16, 1), (32, 1), (64, 1), (64, 2), (64, 3), (64, 5)}
    for dtype, C in [("bf16", 20), ("bf16", 37), ("fp32", 37)]:
        assert L.plan(C, dtype)[0] == "scalar"
    assert L.plan(256, "bf16", (256,), (4096 + 2,))[0] == "scalar"   # base one element off
    assert L.plan(256, "fp32", (256,), (4096 + 4,))[0] == "scalar"
    assert L.plan(256, "bf16", (257, 256), (4096,))[0] == "scalar"   # row stride C + 1
    assert L.plan(256, "bf16", (264, 256), (4096,)) == ("vec", 32, 1)  # row stride C + 8
    assert 14 * 8 == 112 and 16 - 14 == 2                             # bf16 112: two dead lanes of 16
    assert 5 * 64 * 4 - 896 == 384                                    # fp32 896: K = 5 leaves a dead chunk


# ------------------------------------------------------------------ float64 models == torch float64
@pytest.mark.parametrize("dtype,C", [("bf16", 8), ("bf16", 112), ("fp32", 37), ("bf16", 256), ("fp32", 1280)])
@pytest.mark.parametrize("eps", L.EPS)
def test_float64_models_are_torch_layer_norm(dtype, C, eps):
    x, _ = L.make_rows(C, dtype)
    gamma, beta = L.make_params(C)
    dy = L.make_noise(L.NROWS, C, dtype, 1)
    dres = L.make_noise(L.NROWS, C, dtype, 2)
    dg0, db0 = L.make_noise(2, C, "fp32", 3)
    e = L.f32(eps)
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    gt = torch.tensor(gamma, dtype=torch.float64, requires_grad=True)
    bt = torch.tensor(beta, dtype=torch.float64, requires_grad=True)
    yt = torch.nn.functional.layer_norm(xt, (C,), gt, bt, e)
    yt.backward(torch.tensor(dy, dtype=torch.float64))
    y, mean, rstd = L.fwd64(x, gamma, beta, eps)
    dx, dg, db = L.bwd64(x, dy, gamma, eps, addend=dres, dg0=dg0, db0=db0)

    def close(a, b, what):
        # float64 against float64: 1e-11 of each row / column's own size (rstd up to 1e3 amplifies 1e-16)
        a, b = np.asarray(a, F64), np.asarray(b, F64)
        scale = np.abs(b).max(axis=-1, keepdims=True) if b.ndim > 1 else np.abs(b)
        assert np.all(np.abs(a - b) <= 1e-11 * scale + 1e-13), what

    close(y, yt.detach().numpy(), "y")
    close(mean, x.astype(F64).mean(axis=1), "mean")
    close(rstd, 1 / np.sqrt(x.astype(F64).var(axis=1) + e), "rstd")
    close(dx, xt.grad.numpy() + dres, "dx + dres")
    # a column of dgamma sums rows whose xhat is conditioned by rstd max|x| (up to 2e3): 1e-14 of that
    cond = (np.abs(dy.astype(F64)) * (1 + rstd * np.abs(x).max(axis=1))[:, None]).sum(axis=0)
    assert np.all(np.abs(dg - dg0 - gt.grad.numpy()) <= 1e-14 * cond), "dgamma"
    close(db - db0, bt.grad.numpy(), "dbeta")
    v = np.linspace(-6, 6, 25)
    close(L.gelu64(v), torch.nn.functional.gelu(torch.tensor(v)).numpy(), "gelu")


def test_bf16_rounding_is_torch():
    g = np.random.default_rng(1)
    v = np.concatenate([g.standard_normal(4096) * 10.0 ** g.integers(-6, 6, 4096), [301.0, 303.0, 0.0, -0.0]])
    v = v.astype(np.float32)
    assert np.array_equal(L.round_bf16(v), torch.tensor(v).to(torch.bfloat16).float().numpy())


# ------------------------------------------------------------------ the clean model holds everything
@pytest.mark.parametrize("dtype,C", L.SIZES, ids=SIZE_IDS)
def test_clean_model_within_quarter(dtype, C):
    """<= 0.25 of every tolerance on the fp32 value, <= 1 once the output is rounded to the storage type
    (rounding alone reaches half an ulp, which is the whole of rnd())"""
    for G, K, V in _layouts(dtype, C):
        for eps in L.EPS:
            res, names = _run(dtype, C, eps, G, K, V, store=False)
            for k, r in res.items():
                v, where = L.worst(r, names if len(r) == len(names) else None)
                print(f"clean {dtype} C={C} G={G} K={K} VEC={V} eps={eps} {k}: {v:.3f} at {where}")
                assert v <= 0.25, (k, v, where)
            res, names = _run(dtype, C, eps, G, K, V, store=True)
            for k, r in res.items():
                v, where = L.worst(r, names if len(r) == len(names) else None)
                assert v <= 1.0, (k, v, where)


# ------------------------------------------------------------------ every defect breaks a named assertion
def _applicable(defect):
    for dtype, C in L.SIZES:
        for G, K, V in _layouts(dtype, C):
            ok = CATCH[defect][2]
            if ok is None or ok(dtype, C, G, K, V):
                yield dtype, C, G, K, V


@pytest.mark.parametrize("defect", list(L.DEFECTS))
def test_defect_breaks_a_named_assertion(defect):
    """> 10x on one of the named assertions, on one of the named regimes, at every (type, C, lane layout) the
    defect applies to and both eps -- with the outputs rounded to the storage type, as the GPU file sees them"""
    asserts, regimes, _ = CATCH[defect]
    cases = list(_applicable(defect))
    assert cases
    for dtype, C, G, K, V in cases:
        for eps in L.EPS:
            res, names = _run(dtype, C, eps, G, K, V, defects=(defect,))
            best = 0.0
            for a in asserts:
                r = res[a]
                best = max(best, L.worst(r)[0] if regimes is None else
                           max(L.by_regime(r, names)[n] for n in regimes))
            print(f"{defect} {dtype} C={C} G={G} K={K} VEC={V} eps={eps}: {best:.3g}")
            assert best > 10, (defect, dtype, C, (G, K, V), eps, best)


def test_every_regime_is_needed_by_some_defect():
    used = {n for _, regimes, _ in CATCH.values() if regimes for n in regimes}
    assert used == set(L.REGIMES)


# ------------------------------------------------------------------ randn rows do not see them
def _pooled(got, ref):
    """test_kernels_gpu.py _close: max error over the tensor / the tensor's maximum"""
    return float(np.abs(np.asarray(got, F64) - ref).max() / (np.abs(ref).max() + 1e-6))


@pytest.mark.parametrize("dtype,tol", [("fp32", 1e-5), ("bf16", 1e-2)])
@pytest.mark.parametrize("C", [64, 256, 896])
def test_randn_rows_under_the_older_check_pass_the_statistics_defects(dtype, tol, C):
    """test_layernorm's inputs and check (randn rows, eps 1e-6, pooled tolerance) on the defective model"""
    g = np.random.default_rng(C)
    x = L.round_to(g.standard_normal((70, C)).astype(np.float32), dtype)
    a = L.round_to(g.standard_normal((70, C)).astype(np.float32), dtype)
    gamma, beta = g.standard_normal((2, C)).astype(np.float32)
    G, K, V = L.lanes(C, dtype)
    for defect in STAT_DEFECTS:
        y, _, _, xs = L.fwd32(x, gamma, beta, 1e-6, G, K, V, (defect,), add=a, dtype=dtype)
        worst = _pooled(L.round_to(y, dtype), L.fwd64(xs, gamma, beta, 1e-6)[0])
        y, _, _, _ = L.fwd32(x, gamma, beta, 1e-6, G, K, V, (defect,))
        worst = max(worst, _pooled(L.round_to(y, dtype), L.fwd64(x, gamma, beta, 1e-6)[0]))
        print(f"randn {dtype} C={C} {defect}: {worst:.2e} of the maximum (tolerance {tol})")
        if defect == "bessel" and dtype == "fp32":
            assert worst > tol  # 1 / 2C of y: the one statistics defect that fp32 randn rows do see
        else:
            assert worst <= tol, (defect, worst)
    # ... and the same check on the regime rows does not pass them (one_pass, eps_outside; pooled, fp32)
    if dtype == "fp32":
        x, names = L.make_rows(C, dtype)
        for defect, eps in (("one_pass", 1e-6), ("eps_outside", 1e-5)):
            y, _, _, _ = L.fwd32(x, gamma, beta, eps, G, K, V, (defect,))
            ref = L.fwd64(x, gamma, beta, eps)[0]
            rows = [i for i, n in enumerate(names) if n in ("offset30", "const_ulp", "const", "zero", "tiny")]
            assert max(_pooled(y[i:i + 1], ref[i:i + 1]) for i in rows) > 10 * tol, defect
