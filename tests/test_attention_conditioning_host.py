"""The structured attention inputs of attn_cases.py reach what test_attention_conditioning_gpu.py needs them
to reach, proven on the float64 reference alone: which query rows make the flash forward (csrc/flash.hip)
move its reference maximum after tile 0 and how often, which sit just below and just above the trigger,
where probabilities underflow to exactly 0; and a torch model of that forward stays inside the GPU test's
tolerances while the same model without the o *= alpha step misses them by more than 10x."""
import gc
import math

import pytest
import torch

import attn_cases as C

TOL_O, TOL_LSE = 2e-2, 1e-3  # test_attention_conditioning_gpu.py, bf16 paths
H, LQ = 2, 130
SHAPES = [(D, Lk) for D in (56, 72, 256) for Lk in (300, 450)]
_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _release_cache():
    """the shared cases go when the module is done, so the rest of the process does not carry them"""
    yield
    _CACHE.clear()
    gc.collect()


def _case(D, Lk, profile, shift=0.0):
    key = (D, Lk, profile, shift)
    if key not in _CACHE:
        q, k, v = C.make_qkv(1, H, LQ, Lk, D, profile, shift, seed=1)
        ref = C.reference(q, k, v, D ** -0.5)
        _CACHE[key] = (q, k, v, ref, ref["s"][0] * C.LOG2E)  # scores [H, Lq, Lk] in log2 units
    return _CACHE[key]


def _gains(profile, Lk):
    return C.query_gains(LQ, profile, Lk)  # [Lq], as make_qkv used them for this key count


@pytest.mark.parametrize("D,Lk", SHAPES)
def test_ramp_rescales_every_tile_every_second_tile_and_straddles_the_trigger(D, Lk):
    s2 = _case(D, Lk, "ramp")[4]
    count, held, fired = C.regime(s2, detail=True)
    a = _gains("ramp", Lk)
    nfull = Lk // 64  # the ragged last tile adds too little for most rows
    assert (count >= nfull - 1).any(), "no row rescales at every full tile"
    assert (count[:, a == C.SPIKE] >= nfull - 1).all()
    assert (count == nfull // 2).any(), "no row rescales on every second tile"
    assert ((held > 6.0) & (held <= C.RESCALE_LOG2)).any(), "no row comes within 2 log2 units of the trigger"
    assert (fired <= C.RESCALE_LOG2 + 0.25).any(), "no row only just crosses the trigger"
    assert (count[:, a >= 3.9] >= 2).all()
    assert (count[:, a <= 0] == 0).all()  # zero block, gain 0 and the descending ramps of negative gains
    assert (count[:, C.ZERO_ROWS[0]:C.ZERO_ROWS[1]] == 0).all() and (count[:, 16:32] > 0).any() and (count[:, 48:64] > 0).any()


@pytest.mark.parametrize("D,Lk", SHAPES)
def test_ramp_rescales_inside_every_key_split(D, Lk):
    """the key ranges of the GPU test's split launches (flash_plan: 2 splits of 3 tiles at 300 keys, 4 splits
    of 2 tiles at 450) each hold rows that rescale after the split's first tile -- but for the last split of
    450 keys, whose second tile is the 2-key tail"""
    s2 = _case(D, Lk, "ramp")[4]
    tps = 3 if Lk == 300 else 2
    checked = 0
    for t0 in range(0, (Lk + 63) // 64, tps):
        part = s2[..., t0 * 64:(t0 + tps) * 64]
        if part.shape[-1] - 64 < 32:
            continue
        count, _ = C.regime(part)
        assert (count > 0).any(), (t0, tps)
        checked += 1
    assert checked == (2 if Lk == 300 else 3)


@pytest.mark.parametrize("profile", ["saw", "spike_last", "spike_mid"])
@pytest.mark.parametrize("D,Lk", SHAPES)
def test_saw_and_late_spikes_rescale_exactly_once(D, Lk, profile):
    s2 = _case(D, Lk, profile)[4]
    count, _ = C.regime(s2)
    a = _gains(profile, Lk)
    big = a >= 2.5
    assert (count[:, big] == 1).all()
    assert (count[:, a <= 0] == 0).all()
    # ... and late: not before the tile that holds the first large key
    first = 64 if profile == "saw" else C.spike_key(Lk, profile) // 64 * 64
    assert first > 0 and (C.spike_key(Lk, "spike_mid") % 64) != 0
    before, _ = C.regime(s2[..., :first])
    assert (before[:, big] == 0).all()
    if profile == "spike_last":
        assert first == (Lk - 1) // 64 * 64 and Lk % 64 != 0  # the ragged tail tile


@pytest.mark.parametrize("profile", ["spike_first", "flat"])
@pytest.mark.parametrize("D,Lk", SHAPES)
def test_first_key_spike_and_flat_never_rescale(D, Lk, profile):
    count, held = C.regime(_case(D, Lk, profile)[4])
    assert (count == 0).all() and (held <= C.RESCALE_LOG2).all()


@pytest.mark.parametrize("profile", ["spike_first", "spike_last", "spike_mid"])
@pytest.mark.parametrize("D,Lk", SHAPES)
def test_spike_rows_underflow_every_other_key(D, Lk, profile):
    """gain 11 on the spike key's 11: every other key's float64 probability is below 2^-149, the smallest
    fp32 denormal -- its P, and the combine weight of a split without the spike, are exactly 0"""
    _, _, _, ref, s2 = _case(D, Lk, profile)
    rows = _gains(profile, Lk) == C.SPIKE
    assert rows.sum() >= 7
    logp2 = s2 - ref["lse"][0][..., None] * C.LOG2E
    j = C.spike_key(Lk, profile)
    others = torch.ones(Lk, dtype=torch.bool)
    others[j] = False
    assert (logp2[:, rows][..., others] < -149).all()
    assert (logp2[:, rows][..., j].abs() < 1e-9).all()


@pytest.mark.parametrize("shift", C.SHIFTS)
@pytest.mark.parametrize("profile", C.PROFILES)
@pytest.mark.parametrize("D,Lk", SHAPES)
def test_flash_model_is_within_the_gpu_tolerances(D, Lk, profile, shift):
    q, k, v, ref, _ = _case(D, Lk, profile, shift)
    o, lse = C.emulate_flash(q, k, v, D ** -0.5)
    eo = C.row_err(o, ref["o"]).max().item()
    el = (lse.double() - ref["lse"]).abs().max().item()
    print(f"emulate_flash D={D} Lk={Lk} {profile} shift={shift:+.0f}: o {eo:.2e} lse {el:.2e}")
    assert eo <= TOL_O / 4 and el <= TOL_LSE / 20  # measured <= 3.7e-3 and <= 2.5e-5
    if shift:  # the offset moves the LSE and nothing else
        ref0 = _case(D, Lk, profile)[3]
        assert C.row_err(ref["o"], ref0["o"]).max().item() < 1e-9
        assert (ref["lse"] - ref0["lse"] - C.effective_shift(D, shift)).abs().max().item() < 1e-9
        assert abs(C.effective_shift(D, shift) - shift) < 2.0


@pytest.mark.parametrize("profile", ["ramp", "saw", "spike_last"])
@pytest.mark.parametrize("D,Lk", SHAPES)
def test_flash_model_without_the_rescale_misses_by_10x(D, Lk, profile):
    q, k, v, ref, s2 = _case(D, Lk, profile)
    o, _ = C.emulate_flash(q, k, v, D ** -0.5, skip_rescale=True)
    err = C.row_err(o, ref["o"])[0].t()  # [H, Lq]
    count, _ = C.regime(s2)
    print(f"skip_rescale D={D} Lk={Lk} {profile}: o error of the rescaling rows {err[count > 0].min().item():.2e}"
          f" .. {err.max().item():.2e}")
    assert err.max().item() >= 10 * TOL_O
    assert (err[count == 0] <= TOL_O / 4).all()  # only the rows that rescale can see the fault
    if profile != "ramp":  # (a ramp row's first rescale can come while o is still tiny)
        assert (err[count > 0] > TOL_O).all()
    if profile == "spike_last":
        assert (err[count > 0] >= 10 * TOL_O).all()


@pytest.mark.parametrize("profile", C.PROFILES)
@pytest.mark.parametrize("D,Lk", SHAPES)
def test_backward_model_is_within_the_gpu_gradient_tolerance(D, Lk, profile):
    """the bf16 recomputing backward in torch against float64 autograd, per tensor relative to max |ref| as the
    GPU test compares: within 4e-2 (the flash paths' bound) with a factor 1.5 to spare on the unshifted cases
    (measured: dq <= 2.2e-2 on the ramp, <= 1.8e-2 elsewhere; dk <= 6.8e-3; dv <= 4.4e-3); with the +-60 offset
    dk and dv keep that margin while dq reaches 4.6e-2 -- bf16 dS times the enlarged keys -- which is why the
    GPU test does not assert the shifted dq of the bf16 paths.  Most of the unshifted dq error is D_i taken
    from the bf16-rounded O (o_fp32 shows it); the spike profiles' half-mass rows (query_gains) keep the
    tensor maximum it is measured against from being left to chance"""
    tol_g = 4e-2
    do = torch.randn(1, LQ, H, D, generator=torch.Generator().manual_seed(7)).bfloat16()
    for shift in C.SHIFTS:
        q, k, v, _, _ = _case(D, Lk, profile, shift)
        ref = C.reference(q, k, v, D ** -0.5, do=do)
        err = {n: C.tensor_err(g, ref[n]) for g, n in zip(C.emulate_flash_bwd(q, k, v, do, D ** -0.5), ("dq", "dk", "dv"))}
        print(f"emulate_flash_bwd D={D} Lk={Lk} {profile} shift={shift:+.0f}: " + " ".join(f"{n} {e:.2e}" for n, e in err.items()))
        assert err["dk"] <= tol_g / 1.5 and err["dv"] <= tol_g / 1.5
        if not shift:
            assert err["dq"] <= tol_g / 1.5
            if profile.startswith("spike"):
                assert ref["dq"].abs().max().item() > 0.5  # the half-mass rows set the scale


def test_key_profiles_and_gains():
    a = C.query_gains(LQ, "saw")
    assert set(C.GAINS) >= {0.0, 1.0, 2.5, 3.9, 4.0, 6.3, -4.0, -6.3} and a[8:16].tolist() == C.GAINS
    assert (a[32:48] == 0).all() and (C.query_gains(LQ, "spike_mid") == C.SPIKE).sum() == 7
    assert C.SPIKE * C.SPIKE * C.LOG2E > 149
    for Lk in (300, 450, 20, 8):
        for p in C.PROFILES:
            assert C.key_profile(Lk, p).shape == (Lk,)
        assert C.key_profile(Lk, "ramp")[-1] == 6.3 and C.key_profile(Lk, "flat").abs().max() == 0
        assert C.key_profile(Lk, "spike_last").nonzero().flatten().tolist() == [Lk - 1]
    saw = C.key_profile(300, "saw")
    assert saw[:64].max() == 0 and saw[64:128].min() == 6.3 and saw[256:].min() == 0


@pytest.mark.parametrize("D", [16, 32, 56, 64, 72, 96, 256])
def test_inputs_are_exact_in_bf16_and_fp32_alike(D):
    qb, kb, vb = C.make_qkv(1, 2, 24, 70, D, "spike_mid", -60.0, seed=3)
    qf, kf, vf = C.make_qkv(1, 2, 24, 70, D, "spike_mid", -60.0, seed=3, dtype=torch.float32)
    assert qb.dtype == torch.bfloat16 and qf.dtype == torch.float32
    assert torch.equal(qb.float(), qf) and torch.equal(kb.float(), kf) and torch.equal(vb, vf.bfloat16())
    s = C.reference(qb, kb, vb, D ** -0.5)["s"]
    assert abs(s.median().item() - C.effective_shift(D, -60.0)) < 1.0
    assert math.isclose(C.effective_shift(D, 60.0), -C.effective_shift(D, -60.0))
