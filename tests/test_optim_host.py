"""The optimizer step without a GPU: csrc/optim_elem.h compiled for the host (csrc/optim_host_check.cpp: a
stand-alone program, built with -ffp-contract=off plain and under the address and undefined-behaviour sanitizers),
the numpy fp32 model and the float64 reference of optim_cases.py.

* the reference is clip_grad_norm_ + torch.optim.AdamW(foreach=False) in float64 on the CPU, to float64 rounding
  (with torch's float64 decay scalar; everywhere else it uses float32(1 - lr * wd), what torch applies to an fp32
  parameter), and poisons the elements torch poisons when one gradient is inf or NaN;
* the model equals the host check bit for bit on every case, for both builds;
* the model stays close to the reference, each step started from the model's own fp32 state.  Measured over all
  cases, the model's worst error (a measurement of the model against the reference, never of the kernel):

      p   17.2   (size-4099)         in units of ulp(p_ref) + 2^-23 |p_ref - p_before|
      m   1.51   (zero-state-mixed)  in units of ulp(m_ref) + 2^-23 |m_ref - m_before|
      v   1.76   (zero-state-mixed)  in units of ulp(v_ref) + 2^-23 |v_ref - v_before|

  (p's worst element is one whose m cancels to a small value: the update inherits that m's rounding, which is
  counted against the far smaller change of p.)  The bounds are four times these, rounded up (BOUND: 69, 7, 8);
  the room covers the decay scalar landing on the other fp32
  neighbour of torch's (decay-neighbour provokes it: fma(-float(lr), wd, 1) against float32(1 - lr * wd) with a
  double lr), which stays inside the ulp(p) term;
* every mutant of optim_cases.MUTANTS misses a bound by at least 10x on a named case, and the contracted
  `g * cf - m` differs from the model in at least one bit on the inexact-clip case;
* the norm: out[0] may differ from the float64 norm by norm_depth(n) * 2^-24 relative -- the count is written out in
  optim_cases.norm_depth: 20 for N_BIG on the 16-B path, 33 on the scalar path -- and the model's summation tree
  sits under it on the randn and the 1e-12 cases.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import optim_cases as OC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sam2-video-training_amd", "csrc")
F = np.float32

MEASURED = {"p": 17.2, "m": 1.51, "v": 1.76}  # see the module docstring
BOUND = {k: float(np.ceil(4 * x)) for k, x in MEASURED.items()}


@pytest.fixture(scope="module")
def cases():
    return OC.make_cases()


@pytest.fixture(scope="module")
def runs(cases):
    """per case the model's trajectory [(g, before, model step, reference step)] -- computed once, never changed"""
    return {c["name"]: trajectory(c) for c in cases}


def trajectory(case, mutant=None):
    out = []
    p, m, v = case["p"], case["m"], case["v"]
    for k in range(case["steps"]):
        ref = OC.reference_step(case, k, p, m, v)
        mod = OC.model_step(case, k, p, m, v, mutant)
        out.append(((p, m, v), mod, ref))
        p, m, v = mod[2:]
    return out


def worst_units(traj):
    w = {"p": 0.0, "m": 0.0, "v": 0.0}
    for before, mod, ref in traj:
        for i, key in enumerate("pmv"):
            w[key] = max(w[key], float(OC.error_units(mod[2 + i], ref[2 + i], before[i]).max()))
    return w


# ------------------------------------------------------------------------------------------------ the host check
@pytest.fixture(scope="module", params=["plain", "sanitized"])
def host_check(request, tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build csrc/optim_host_check.cpp")
    exe = tmp_path_factory.mktemp("optim_host") / f"optim_host_check_{request.param}"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", *flags, "-I", CSRC,
                    os.path.join(CSRC, "optim_host_check.cpp"), "-o", str(exe)], check=True)
    return str(exe)


def run_host(exe, records, tmp_path):
    """records: (n, step, [lr, beta1, beta2, eps, wd, sumsq, max_norm, grad_scale], p, g, m, v) -> per record
    (clip pair, derived scalars, p, m, v, shadow bits)"""
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        for n, step, sc, p, g, m, v in records:
            f.write(np.asarray([n, step], np.int32).tobytes())
            f.write(np.asarray(sc, F).tobytes())
            for a in (p, g, m, v):
                assert a.dtype == F and a.size == n
                f.write(a.tobytes())
    res = subprocess.run([exe, str(src), str(dst)], timeout=600, capture_output=True, text=True)
    assert res.returncode == 0 and res.stderr == "", (res.returncode, res.stderr[-2000:])
    raw = dst.read_bytes()
    out, off = [], 0
    for n, *_ in records:
        clip = np.frombuffer(raw, F, 2, off)
        derived = np.frombuffer(raw, F, 5, off + 8)
        off += 28
        p, m, v = (np.frombuffer(raw, F, n, off + 4 * n * i) for i in range(3))
        off += 12 * n
        sh = np.frombuffer(raw, np.uint16, n, off)
        off += 2 * n
        out.append((clip, derived, p, m, v, sh))
    assert off == len(raw)
    return out


def bits(a):
    return np.asarray(a, F).view(np.uint32)


def same_bits(a, b):
    """bit for bit, any NaN equal to any NaN"""
    a, b = np.asarray(a, F), np.asarray(b, F)
    return bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def host_records(case):
    """the model's trajectory of a case as host-check records, with what the model expects of each"""
    recs, want = [], []
    p, m, v = case["p"], case["m"], case["v"]
    for k in range(case["steps"]):
        g = OC.case_grad(case, k)
        sumsq = OC.model_sumsq(g)
        step = case["step0"] + k
        recs.append((case["n"], step, [case["lr"], case["beta1"], case["beta2"], case["eps"], case["wd"], sumsq,
                                       case["max_norm"], case["grad_scale"]], p, g, m, v))
        mod = OC.model_step(case, k, p, m, v)
        sc = OC.model_scalars(case["lr"], case["beta1"], case["beta2"], case["wd"], step)
        want.append((mod, [sc[key] for key in ("step_size", "bc2_sqrt", "decay", "w1", "omb2")]))
        p, m, v = mod[2:]
    return recs, want


def check_host(exe, cs, tmp_path):
    recs, want, names = [], [], []
    for c in cs:
        r, w = host_records(c)
        recs += r
        want += w
        names += [f"{c['name']} step {c['step0'] + k}" for k in range(c["steps"])]
    got = run_host(exe, recs, tmp_path)
    for name, (clip, derived, p, m, v, sh), (mod, sc) in zip(names, got, want):
        assert same_bits(clip, mod[:2]), (name, clip, mod[:2])
        assert same_bits(derived, sc), (name, derived, sc)
        for key, a, b in zip("pmv", (p, m, v), mod[2:]):
            assert same_bits(a, b), (name, key, int((bits(a) != bits(b)).sum()))
        assert (sh == OC.bf16_bits(mod[2])).all(), name


def test_model_equals_the_header_on_the_host(host_check, cases, tmp_path):
    check_host(host_check, cases + OC.make_nonfinite_cases(), tmp_path)


def test_model_equals_the_header_on_the_big_case(host_check, tmp_path):
    check_host(host_check, [OC.make_big_case()], tmp_path)


def test_host_check_refuses_bad_sizes(host_check, tmp_path):
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(np.asarray([-1, 1], np.int32).tobytes() + np.zeros(8, F).tobytes())
    assert subprocess.run([host_check, str(src), str(dst)], timeout=60).returncode == 3


# ------------------------------------------------------------------------------------------------ model pieces
def test_fmaf_emulation_is_exact():
    """a random sample against exact rational arithmetic, and sums that need more than float64's 53 bits: the
    product 8392705 * 8384513 = 2^46 + 1 puts one bit 46 places below a tie of the fp32 result"""
    from fractions import Fraction
    rng = np.random.default_rng(1)
    a, b, c = (rng.standard_normal(100_000).astype(F) for _ in range(3))
    c *= F(1e-3)
    got = OC.fmaf(a, b, c)
    for i in range(0, a.size, 499):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        d = abs(Fraction(float(got[i])) - exact)
        for other in (np.nextafter(got[i], F(-np.inf)), np.nextafter(got[i], F(np.inf))):
            assert d < abs(Fraction(float(other)) - exact)
    x, y = F(8392705.0), F(8384513.0 * 2.0 ** -40)
    assert float(x) * float(y) == 64.0 + 2.0 ** -40
    assert F(float(x) * float(y) + 2.0 ** 30) == F(2.0 ** 30)           # float64 first: the tie, to even
    assert OC.fmaf(x, y, F(2.0 ** 30)) == F(2.0 ** 30 + 128.0)          # above the tie
    assert F(float(x) * -float(y) + (2.0 ** 30 + 256.0)) == F(2.0 ** 30 + 256.0)
    assert OC.fmaf(x, -y, F(2.0 ** 30 + 256.0)) == F(2.0 ** 30 + 128.0)  # below the tie
    assert OC.fmaf(F(2.0 ** -24), F(1.0), F(1.0)) == F(1.0)             # an exact tie goes to even
    assert OC.fmaf(F(3 * 2.0 ** -24), F(1.0), F(1.0)) == F(1.0 + 2.0 ** -22)
    assert not np.signbit(OC.fmaf(F(-1e-3), F(0.0), F(0.0))) and np.signbit(OC.fmaf(F(-1e-3), F(0.0), F(-0.0)))
    assert np.isnan(OC.fmaf(F(np.inf), F(0.0), F(1.0))) and OC.fmaf(F(np.inf), F(1.0), F(1.0)) == np.inf
    assert OC.fmaf(F(2.0 ** -100), F(2.0 ** -49), F(0.0)) == F(2.0 ** -149)  # the smallest denormal
    assert OC.fmaf(F(2.0 ** -100), F(2.0 ** -50), F(0.0)) == F(0.0)          # half of it: the tie, to even


def test_bf16_bits_are_torch_rounding():
    rng = np.random.default_rng(2)
    x = np.concatenate([rng.standard_normal(10_000).astype(F) * F(3.0), np.asarray([0.0, -0.0, 1e-40, 3e38], F)])
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert (OC.bf16_bits(x) == want).all()


# ------------------------------------------------------------------------------------------------ the reference
def _torch_step(case, k, p, m, v):
    """clip_grad_norm_ + torch.optim.AdamW(foreach=False) in float64 from the state (p, m, v)"""
    g = OC.case_grad(case, k).astype(np.float64) * OC.abi(case["grad_scale"])
    step = case["step0"] + k
    pt = torch.nn.Parameter(torch.from_numpy(np.asarray(p, np.float64).copy()))
    opt = torch.optim.AdamW([pt], lr=case["lr"], betas=(OC.abi(case["beta1"]), OC.abi(case["beta2"])),
                            eps=OC.abi(case["eps"]), weight_decay=case["wd"], foreach=False)
    opt.state[pt] = {"step": torch.tensor(float(step - 1)),
                     "exp_avg": torch.from_numpy(np.asarray(m, np.float64).copy()),
                     "exp_avg_sq": torch.from_numpy(np.asarray(v, np.float64).copy())}
    pt.grad = torch.from_numpy(g.copy())
    total = None
    if OC.abi(case["max_norm"]) > 0:
        total = float(torch.nn.utils.clip_grad_norm_([pt], OC.abi(case["max_norm"]), foreach=False))
    opt.step()
    st = opt.state[pt]
    return total, pt.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()


def _close64(a, b, scale):
    """to float64 rounding: 64 float64 epsilons of the operands' size"""
    a, b, scale = (np.asarray(x, np.float64) for x in (a, b, scale))
    return bool((np.abs(a - b) <= 64 * np.finfo(np.float64).eps * np.maximum(scale, np.finfo(np.float64).tiny)).all())


def test_reference_is_torch_in_float64(cases):
    """each value against the size of the operands it is formed from: m and v against max(|new|, |old|) (a moment
    that cancels keeps the rounding of its operands), p against that plus the update's operands,
    step_size * max(|m_old|, |m_new|, |g|) / denom"""
    for c in cases:
        p, m, v = c["p"], c["m"], c["v"]
        for k in range(c["steps"]):
            total, factor, pr, mr, vr = OC.reference_step(c, k, p, m, v, decay32=False)
            tt, pt, mt, vt = _torch_step(c, k, p, m, v)
            if tt is not None:
                assert abs(tt - total) <= 1e-14 * total, c["name"]
            step = c["step0"] + k
            b1, b2 = OC.abi(c["beta1"]), OC.abi(c["beta2"])
            denom = np.sqrt(vr) / np.sqrt(1.0 - b2 ** step) + OC.abi(c["eps"])
            gc = np.abs(OC.case_grad(c, k).astype(np.float64) * factor)
            upd = c["lr"] / (1.0 - b1 ** step) * np.maximum(np.maximum(np.abs(m), np.abs(mr)), gc) / denom
            assert _close64(mr, mt, np.maximum(np.abs(mr), np.abs(m))), c["name"]
            assert _close64(vr, vt, np.maximum(np.abs(vr), np.abs(v))), c["name"]
            assert _close64(pr, pt, np.maximum(np.abs(pr), np.abs(p)) + upd), c["name"]
            p, m, v = OC.model_step(c, k, p, m, v)[2:]


def test_reference_poisons_what_torch_poisons():
    for c in OC.make_nonfinite_cases():
        _, _, pr, mr, vr = OC.reference_step(c, 0, c["p"], c["m"], c["v"], decay32=False)
        _, pt, mt, vt = _torch_step(c, 0, c["p"], c["m"], c["v"])
        for a, b in ((pr, pt), (mr, mt), (vr, vt)):
            assert (np.isfinite(a) == np.isfinite(b)).all() and (np.isnan(a) == np.isnan(b)).all(), c["name"]
        bad = ~np.isfinite(pr)
        if c["max_norm"] == 0 or c["name"].startswith("inf"):
            assert bad.sum() == 1 and bad[c["poison_at"]], c["name"]  # the one element
        else:
            assert bad.all(), c["name"]  # a NaN norm poisons every element
        # the model poisons the same elements
        _, _, pm, mm, vm = OC.model_step(c, 0, c["p"], c["m"], c["v"])
        assert (np.isnan(pm) == np.isnan(pr)).all() and (np.isfinite(mm) == np.isfinite(mr)).all(), c["name"]
        assert (np.isfinite(vm) == np.isfinite(vr)).all(), c["name"]


# ------------------------------------------------------------------------------------------------ model vs reference
def test_cases_cover_what_they_claim(cases, runs):
    by = {c["name"]: c for c in cases}
    factor = {name: [float(ref[1]) for _, _, ref in tr] for name, tr in runs.items()}
    norm = {name: [float(ref[0]) for _, _, ref in tr] for name, tr in runs.items()}
    assert factor["clip-under"] == [1.0] and norm["clip-under"][0] < 0.1          # the clamp is taken
    assert factor["clip-over"][0] < 0.1 and factor["clip-tiny-over"][0] < 0.5
    assert norm["clip-equal"] == [1.0] and 0.999998 < factor["clip-equal"][0] < 1.0
    assert norm["clip-zero-grad"] == [0.0] and factor["clip-zero-grad"] == [1.0]
    assert factor["clip-off"] == [1.0] and norm["clip-off"][0] > 1.0
    assert factor["zero-state-g1"][0] < 0.1 and all(f == [1.0] * 5 for f in
                                                    (factor[f"zero-state-g{s:g}"] for s in OC.GRAD_SCALES[1:]))
    assert {c["grad_scale"] for c in cases} >= {1.0, 0.5, 1.0 / 3.0, 1.0 / 16.0, 0.7}
    assert {c["step0"] for c in cases} >= {1, 1000, 20_000, 200_000} and {c["n"] for c in cases} >= set(OC.SIZES)
    assert {c["lr"] for c in cases} >= {1e-3, 4e-6, 1e-9, 0.0} and {c["wd"] for c in cases} >= {0.01, 0.0}
    assert 1e-9 * 0.01 < 2.0 ** -25 < 4e-6 * 0.01 and by["beta1-0"]["beta1"] == 0.0
    # the decay scalar on the other neighbour of torch's
    c = by["decay-neighbour"]
    d, torchs = OC.model_scalars(c["lr"], 0.9, 0.999, c["wd"], 1)["decay"], F(1.0 - c["lr"] * c["wd"])
    assert d != torchs and abs(float(d) - float(torchs)) == 2.0 ** -24
    # eps dominates / g^2 denormal; zeros against moments; all-zero elements; signed zeros in p
    c = by["zero-state-g1e-20"]
    g = OC.case_grad(c, 0)
    g2 = g.astype(np.float64) ** 2
    assert ((g2 > 0) & (g2 < 2.0 ** -126)).any()
    c = by["carried-1000-zeros"]
    g = OC.case_grad(c, 0)
    assert ((g == 0) & (c["m"] != 0) & (c["v"] != 0)).any()
    z = (c["p"] == 0) & (g == 0) & (c["m"] == 0) & (c["v"] == 0)
    assert z.any() and np.signbit(c["p"]).any() and (c["p"] == 0).sum() > z.sum()
    assert np.abs(c["p"]).max() == 30.0 and np.abs(c["p"][c["p"] != 0]).min() <= 1.0001e-6
    assert (by["carried-200000-mixed"]["v"] >= 0).all()


def test_model_is_within_the_bounds_of_the_reference(runs):
    worst = {"p": (0.0, ""), "m": (0.0, ""), "v": (0.0, "")}
    for name, tr in runs.items():
        for key, val in worst_units(tr).items():
            if val > worst[key][0]:
                worst[key] = (val, name)
    print("model against the float64 reference, worst units:", worst)
    for key in "pmv":
        assert worst[key][0] <= BOUND[key], (key, worst[key])
        assert worst[key][0] >= MEASURED[key] / 2, ("the docstring's figure is stale", key, worst[key])


def test_all_zero_elements_stay_plus_zero(runs, cases):
    for c in cases:
        p = c["p"]
        z = (p == 0) & ~np.signbit(p) & (c["m"] == 0) & (c["v"] == 0)
        for k, (_, mod, _) in enumerate(runs[c["name"]]):
            z = z & (OC.case_grad(c, k) == 0)
            for a in mod[2:]:
                assert (bits(a[z]) == 0).all(), c["name"]


@pytest.mark.parametrize("mutant", [m for m in OC.MUTANTS if m != "contracted"])
def test_mutant_misses_the_bound_tenfold(mutant, cases):
    caught = {}
    for c in cases:
        w = worst_units(trajectory(c, mutant))
        ratio = max(w[key] / BOUND[key] for key in "pmv")
        if ratio >= 10:
            caught[c["name"]] = ratio
    print(mutant, "caught on", caught)
    assert caught, mutant


def test_contracted_mutant_differs_in_a_bit(cases):
    c = {c["name"]: c for c in cases}["inexact-clip"]
    a = OC.model_step(c, 0, c["p"], c["m"], c["v"])
    b = OC.model_step(c, 0, c["p"], c["m"], c["v"], "contracted")
    assert float(a[1]) == float(F(0.7)) and not same_bits(a[3], b[3])
    assert same_bits(a[4], b[4])  # v does not see it


# ------------------------------------------------------------------------------------------------ the norm
def test_norm_depth_count():
    assert OC.norm_depth(OC.N_BIG, True) == 20 and OC.norm_depth(OC.N_BIG, False) == 33
    assert OC.norm_depth(4099, True) == 18 and OC.norm_depth(1, False) == 15


@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("scale", [1.0, 1e-12])
def test_model_norm_sits_under_the_depth_bound(scale, aligned):
    for n in (4099, OC.N_BIG):
        g = OC._grad(n, np.random.default_rng(n % 1000), "randn", scale)
        got = float(np.sqrt(OC.model_sumsq(g, aligned)))
        want = OC.reference_clip(g, 0.0, 1.0)[0]
        assert abs(got - want) <= OC.norm_tolerance(n, aligned) * want, (n, got, want)


def test_model_norm_is_exact_on_the_pins():
    for n in OC.SIZES + [OC.N_BIG]:
        for aligned in (True, False):
            assert OC.model_sumsq(np.ones(n, F), aligned) == F(n)
            g, total = OC.pin_tensor(n)
            assert OC.model_sumsq(g, aligned) == F(total) and float(F(total)) == total
            for q in OC.pin_positions(n)[:3]:  # one element missed changes the integer
                h = g.copy()
                h[q] = 0
                assert OC.model_sumsq(h, aligned) != F(total)
    assert len(OC.pin_positions(OC.N_BIG)) == 4 + 18
