"""The harness of test_decoder_tok_kernels_gpu.py has teeth (no GPU here): the clean fp32 model of
dec_tok_cases.py holds every assertion on every shape, class and flag -- with a factor 4 to spare on the
value before the output rounding, <= 1 on the bf16-rounded one, equality where claimed -- and each defect of
dec_tok_cases.DEFECTS breaks the assertion DEFECT_SITES names by more than 10x (an equality: breaks it)."""
import numpy as np
import pytest

import dec_tok_cases as dc
import ln_cases as lc

GROUPS = {"proj": tuple(dc.PROJ), "lse": ("lse",), "os": ("os",), "add": dc.ADD_SLOTS,
          "ln y": ("x1", "x2", "x3", "hs"), "ln mean": ("mean1", "mean2", "mean3", "mean"),
          "ln rstd": ("rstd1", "rstd2", "rstd3", "rstd")}
GROUP_OF = {slot: g for g, slots in GROUPS.items() for slot in slots}


@pytest.fixture(scope="module")
def clean():
    """{case: (inputs, out, raw)} of the clean model, computed once"""
    return {c: (dc.build(c),) + dc.model32(c, dc.build(c)) for k in dc.KERNELS for c in dc.cases(k)}


def test_clean_model_within_quarter(clean):
    """run with -s for the worst ratio of each assertion group"""
    top_raw, top_rnd, bad = {}, {}, []
    for c, (inp, out, raw) in clean.items():
        for top, res, limit in ((top_raw, dc.check(c, inp, out, raw), 0.25), (top_rnd, dc.check(c, inp, out), 1.0)):
            for slot, (ratio, row) in dc.worst(res).items():
                g = GROUP_OF[slot]
                if ratio > top.get(g, (-1.0, ""))[0]:
                    top[g] = (ratio, f"{dc.case_id(c)} {slot}[{row}]")
                if not ratio <= limit:
                    bad.append(f"{dc.case_id(c)} {slot}[{row}]: {ratio:.3g} > {limit}")
    for name, top in (("before the output rounding (limit 0.25)", top_raw), ("as stored (limit 1)", top_rnd)):
        print(f"\nclean fp32 model against float64, {name}:")
        for g, (ratio, where) in sorted(top.items()):
            print(f"  {g:8s} {ratio:.3f}  {where}")
    assert not bad, f"{len(bad)} assertion(s) the clean model misses:\n" + "\n".join(bad[:40])
    assert set(top_raw) == set(GROUPS) - {"add"} and set(top_rnd) == set(GROUPS)


def test_clean_model_exact_slots(clean):
    """exact class: the EQUAL_SLOTS are integers the model reproduces bit for bit, and not all zero"""
    n = 0
    for c, (inp, out, _) in clean.items():
        if c.cls != "exact":
            continue
        for slot in dc.EQUAL_SLOTS[c.kernel]:
            v = out[slot]
            assert np.array_equal(v, np.round(v)) and np.abs(v).max() > 8, (c, slot)
            n += 1
    assert n == sum(len(dc.EQUAL_SLOTS[k]) * len([c for c in dc.cases(k) if c.cls == "exact"]) for k in dc.KERNELS)


@pytest.mark.parametrize("defect", list(dc.DEFECTS))
def test_defect_breaks_its_assertion(clean, defect):
    c, slot = dc.DEFECT_SITES[defect]
    assert c in clean, "the named case is not one the GPU file runs"
    inp = clean[c][0]
    out, _ = dc.model32(c, inp, (defect,))
    ratio, row = dc.worst(dc.check(c, inp, out))[slot]
    base = dc.worst(dc.check(c, inp, clean[c][1]))[slot][0]
    print(f"\n{defect}: {dc.case_id(c)} {slot}[{row}] {ratio:.3g} (clean {base:.3g})")
    assert base <= 1 and ratio > 10


def test_every_defect_has_a_site():
    assert set(dc.DEFECTS) == set(dc.DEFECT_SITES)


def test_case_coverage():
    """every shape of the issue's table; every LayerNorm regime in front of every dt_layernorm; objects that
    share a workgroup in different softmax regimes; OUTPUTS holds the 19 bf16 slots, 8 statistics and lse"""
    assert sorted(dc.SHAPES) == sorted([(8, 1), (8, 2), (8, 3), (8, 13), (7, 3), (5, 4), (3, 6), (1, 17), (9, 2), (16, 2)])
    kinds = [kind for v in dc.OUTPUTS.values() for _, kind in v]
    assert (sum(k in (256, 128) for k in kinds), kinds.count("stat"), kinds.count("lse")) == (19, 8, 1)
    for k in dc.KERNELS:
        cs = dc.cases(k)
        assert {(c.T, c.objects) for c in cs} == set(dc.SHAPES)
        assert {c.flag for c in cs} == ({0, 1} if k in ("self", "post_b") else {0})
        assert {c.eps for c in cs if c.cls == "ln"} == set(lc.EPS)
        seen = set()
        for c in cs:
            if c.cls == "ln":
                seen |= set(dc.build(c)["ln_names"])
        assert seen == set(lc.REGIMES), (k, seen)
    for T, O in dc.SHAPES:
        per = dc.ROWS_PER_WG // T
        for o in range(O - 1):
            if (o + 1) % per:  # o and o + 1 share a workgroup
                assert all(dc.sm_regime(o, h) != dc.sm_regime(o + 1, h) for h in range(4))


def test_flat_scores_are_flat():
    """softmax class, flat regime: every score of a row is the same float64 number, p = 1 / T"""
    c = dc.find("self", 5, 4, "softmax", 0)
    inp = dc.build(c)
    out, _ = dc.model32(c, inp)
    r = dc.attn64(c, out["qs"], out["ks"], out["vs"], inp["scale"])
    n = 0
    for o in range(c.objects):
        for h in range(4):
            if dc.sm_regime(o, h) == "flat":
                assert np.allclose(r["p"][o, h], 1.0 / c.T, rtol=1e-12, atol=0)
                n += 1
    assert n >= 3
    # the selection rows copy channels of x + pe
    assert np.array_equal(out["qs"][:, :dc.CI], out["qa"][:, :dc.CI])
    assert np.array_equal(out["ks"][:, :dc.CI], out["qa"][:, dc.CI:])


def test_arena_guards():
    a = dc.Arena(dc.SENT)
    a.add("p", (3, 256), tail=16 * 256)
    a.add("q", (5,), tail=16)
    a.add("r", (2, 8, 3))
    for name in "pqr":
        assert a.offset(name) % 8 == 0 and a.offset(name) >= 16
    flat = a.host({"p": np.ones((3, 256)), "q": np.arange(5), "r": np.zeros((2, 8, 3))})
    got, ok = a.read(flat)
    assert ok and got["q"].tolist() == [0, 1, 2, 3, 4]
    flat[a.offset("p") + 3 * 256] = 1.0   # the first row past R
    assert not a.read(flat)[1]
    flat[a.offset("p") + 3 * 256] = dc.SENT
    flat[a.offset("q") - 1] = 0.0         # a guard
    assert not a.read(flat)[1]
