"""The optimizer step on the device (csrc/optim.hip s2h_grad_norm / s2h_adamw, training/optim.py ArenaAdamW) against
the fp32 model and the float64 reference of optim_cases.py (test_optim_host.py shows on the CPU that the model is
csrc/optim_elem.h bit for bit, how far it is from the reference, and that the cases tell wrong formulas apart).

* out[0] bit for bit on the exact pins (all ones; zeros with powers of two where a missed or doubled element would
  hide, where also the 1024 partial sums add up to the exact integer), within norm_depth * 2^-24 of the float64
  norm elsewhere; out[1] bit-equal to the header's formula on the device's own out[0];
* p, m, v and the bf16 shadow bit-equal to the model (which takes the device's out[1]) on every step of every
  case, 16-B aligned and at a one-float offset, the shadow 8-B aligned, misaligned and absent, N_BIG included;
  the shadow also equals torch's p.to(bfloat16); all-zero elements stay +0; nothing outside a view is written;
* an inf / NaN gradient poisons exactly the reference's elements;
* ArenaAdamW.step on a two-parameter arena with alignment padding, with and without a shadow, agrees with the model.
"""
import numpy as np
import pytest
import torch

import optim_cases as OC
from sam2_video.kernels import ops
from sam2_video.kernels.arena import ParamArena
from sam2_video.training.optim import ArenaAdamW

pytestmark = pytest.mark.gpu

F = np.float32
DEV = "cuda"
FILL = {torch.float32: 7.0, torch.bfloat16: 5.0}
# (offset of the fp32 views in floats past a 16-B boundary, offset of the shadow in bf16 past an 8-B boundary or
# None): the 16-B kernel + scalar tail; the scalar kernel because of the shadow's / the arrays' alignment; no shadow
LAYOUTS = {"vector": (0, 0), "shadow-misaligned": (0, 1), "offset": (1, 0), "offset-both": (1, 3),
           "no-shadow": (0, None)}


class View:
    """n elements inside a sentinel-filled buffer, `shift` elements past an aligned start"""

    def __init__(self, n, shift, dtype=torch.float32, src=None):
        self.lo, self.n = 8 + shift, n
        self.buf = torch.full((n + 24,), FILL[dtype], device=DEV, dtype=dtype)
        self.t = self.buf[self.lo:self.lo + n]
        if src is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(src)))

    def host(self):
        t = self.t.cpu()
        return (t.view(torch.int16).numpy().view(np.uint16) if t.dtype == torch.bfloat16 else t.numpy())

    def untouched_outside(self):
        b, fill = self.buf.cpu().float(), FILL[self.buf.dtype]
        return bool((b[:self.lo] == fill).all() and (b[self.lo + self.n:] == fill).all())


def bits(a):
    return np.asarray(a, F).view(np.uint32)


def same_bits(a, b):
    a, b = np.asarray(a, F), np.asarray(b, F)
    return bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def grad_norm(g, max_norm, grad_scale):
    """(out, the 1024 partial sums) of s2h_grad_norm, on the host"""
    ws, out = torch.zeros(1024, device=DEV), torch.full((4,), 7.0, device=DEV)
    ops.grad_norm(g, max_norm, ws, out[1:3], grad_scale)
    o = out.cpu().numpy()
    assert o[0] == 7.0 and o[3] == 7.0
    return o[1:3].copy(), ws.cpu().numpy()


@pytest.fixture(scope="module")
def cases():
    return OC.make_cases()


# ------------------------------------------------------------------------------------------------ the norm
@pytest.mark.parametrize("shift", [0, 1])
def test_norm_exact_pins(shift):
    for n in OC.SIZES + [OC.N_BIG]:
        ones = View(n, shift, src=np.ones(n, F))
        out, ws = grad_norm(ones.t, 0.0, 1.0)
        assert bits(out[0]) == bits(np.sqrt(F(n))) and out[1] == 1.0, (n, out)
        assert ws.astype(np.float64).sum() == n and ones.untouched_outside() and (ones.host() == 1).all()
        g, total = OC.pin_tensor(n)
        pins = View(n, shift, src=g)
        out, ws = grad_norm(pins.t, 0.0, 1.0)
        assert ws.astype(np.float64).sum() == total, (n, ws.astype(np.float64).sum(), total)
        assert bits(out[0]) == bits(np.sqrt(F(total))), (n, out)


@pytest.mark.parametrize("shift", [0, 1])
def test_norm_within_the_depth_bound_and_factor_from_the_header(shift, cases):
    """every case's first gradient, and N_BIG of randn at scale 1 and 1e-12 (max_norm 1: one clips, one does not)"""
    extra = [dict(name=f"big-{s:g}", n=OC.N_BIG, max_norm=1.0, grad_scale=1.0 / 3.0,
                  grad_fn=lambda k, _s=s: OC._grad(OC.N_BIG, np.random.default_rng(7), "randn", _s))
             for s in (1.0, 1e-12)]
    seen = set()
    for c in cases + extra:
        g = OC.case_grad(c, 0)
        total, factor = OC.reference_clip(g, OC.abi(c["max_norm"]), OC.abi(c["grad_scale"]))
        out, _ = grad_norm(View(c["n"], shift, src=g).t, c["max_norm"], c["grad_scale"])
        tol = OC.norm_tolerance(c["n"], aligned=shift == 0)
        allowed = tol * total + (OC.norm_underflow(c["n"]) / total if total > 0 else 0.0)
        err = abs(float(out[0]) - total)
        print(c["name"], shift, "out[0]", out[0], "float64", total, "error", err, "allowed", allowed)
        assert err <= allowed, (c["name"], out, total)
        want = OC.model_clip_factor(out[0], c["max_norm"], c["grad_scale"])
        assert bits(out[1]) == bits(want), (c["name"], out, want)
        # and the factor itself: the norm's bound and the three roundings of the formula
        rel = allowed / max(total, 1e-300) + 3 * 2.0 ** -24
        assert abs(float(out[1]) - factor) <= rel * abs(factor), (c["name"], out, factor)
        seen.add(float(out[1]) == float(F(c["grad_scale"])))
    assert seen == {True, False}  # the clamp (or no clip) and a real clip both occurred


# ------------------------------------------------------------------------------------------------ AdamW
def device_trajectory(case, layout, check_reference=None):
    """runs every step of a case on the device, asserting each against the model: p, m, v, shadow bit for bit"""
    shift, sh_shift = LAYOUTS[layout]
    n = case["n"]
    p, m, v = (View(n, shift, src=case[k]) for k in "pmv")
    sh = View(n, sh_shift, torch.bfloat16) if sh_shift is not None else None
    ws, out = torch.zeros(1024, device=DEV), torch.zeros(2, device=DEV)
    mp, mm, mv = case["p"], case["m"], case["v"]
    zero = (bits(mp) == 0) & (bits(mm) == 0) & (bits(mv) == 0)
    for k in range(case["steps"]):
        g0 = OC.case_grad(case, k)
        g = View(n, shift, src=g0)
        ops.grad_norm(g.t, case["max_norm"], ws, out, case["grad_scale"])
        ops.adamw(p.t, g.t, m.t, v.t, out, case["lr"], case["beta1"], case["beta2"], case["eps"], case["wd"],
                  case["step0"] + k, sh.t if sh is not None else None)
        pair = out.cpu().numpy()
        before = (mp, mm, mv)
        _, _, mp, mm, mv = OC.model_step(case, k, mp, mm, mv, clip_pair=(pair[0], pair[1]))
        tag = (case["name"], layout, case["step0"] + k)
        for key, dev, want in (("p", p, mp), ("m", m, mm), ("v", v, mv)):
            got = dev.host()
            assert same_bits(got, want), tag + (key, int((bits(got) != bits(want)).sum()))
            assert dev.untouched_outside(), tag + (key,)
        assert same_bits(g.host(), g0) and g.untouched_outside(), tag
        if sh is not None:
            got = sh.host()
            ok = (got == OC.bf16_bits(mp)) | np.isnan(mp)
            assert ok.all() and sh.untouched_outside(), tag
            torchs = p.t.to(torch.bfloat16).cpu()
            assert torch.equal(sh.t.cpu().view(torch.int16)[~torch.isnan(torchs)],
                               torchs.view(torch.int16)[~torch.isnan(torchs)]), tag
            assert bool(torch.isnan(sh.t.cpu()[torch.isnan(torchs)]).all()), tag
        zero = zero & (g0 == 0) & bool(np.isfinite(pair[1]))  # (a NaN factor poisons zeros too)
        for a in (mp, mm, mv):
            assert (bits(a)[zero] == 0).all(), tag  # the model's all-zero elements stay +0, so the device's do
        if check_reference is not None:
            check_reference(case, k, before, (p.host(), m.host(), v.host()))
    return zero


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_adamw_is_the_model_bit_for_bit(layout, cases):
    stayed_zero = 0
    for c in cases:
        stayed_zero += int(device_trajectory(c, layout).sum())
    assert stayed_zero > 100


@pytest.fixture(scope="module")
def big():
    c = OC.make_big_case()
    want = OC.model_step(c, 0, c["p"], c["m"], c["v"], clip_pair=(F(0.0), F(0.7)))[2:]
    return c, want


@pytest.mark.parametrize("layout", ["vector", "offset"])
def test_adamw_big_case_is_the_model_bit_for_bit(layout, big):
    """N_BIG: a second grid-stride round of the 16-B kernel, nine of the scalar kernel; the factor is 0.7f whatever
    the norm (max_norm 0, grad_scale 0.7), so one model run serves both layouts"""
    c, want = big
    shift, sh_shift = LAYOUTS[layout]
    n = c["n"]
    p, m, v = (View(n, shift, src=c[k]) for k in "pmv")
    g = View(n, shift, src=OC.case_grad(c, 0))
    sh = View(n, sh_shift, torch.bfloat16)
    ws, out = torch.zeros(1024, device=DEV), torch.zeros(2, device=DEV)
    ops.grad_norm(g.t, c["max_norm"], ws, out, c["grad_scale"])
    ops.adamw(p.t, g.t, m.t, v.t, out, c["lr"], c["beta1"], c["beta2"], c["eps"], c["wd"], c["step0"], sh.t)
    assert bits(out.cpu().numpy()[1]) == bits(F(0.7))
    for key, dev, w in (("p", p, want[0]), ("m", m, want[1]), ("v", v, want[2])):
        got = dev.host()
        assert same_bits(got, w), (layout, key, int((bits(got) != bits(w)).sum()))
        assert dev.untouched_outside(), (layout, key)
    assert (sh.host() == OC.bf16_bits(want[0])).all() and sh.untouched_outside() and g.untouched_outside()
    assert torch.equal(sh.t, p.t.to(torch.bfloat16))


@pytest.mark.parametrize("layout", ["vector", "offset"])
def test_nonfinite_gradient_poisons_the_references_elements(layout):
    def check(case, k, before, got):
        ref = OC.reference_step(case, k, *before)[2:]
        for a, r in zip(got, ref):
            assert (np.isnan(a) == np.isnan(r)).all() and (np.isfinite(a) == np.isfinite(r)).all(), case["name"]
        bad = ~np.isfinite(got[0])
        if case["max_norm"] == 0 or case["name"].startswith("inf"):
            assert bad.sum() == 1 and bad[case["poison_at"]]
        else:
            assert bad.all()

    for c in OC.make_nonfinite_cases():
        device_trajectory(c, layout, check)


# ------------------------------------------------------------------------------------------------ the arena
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_arena_adamw_step_is_the_model(dtype):
    """two trainable parameters (231 and 33 elements: 25 + 31 elements of alignment padding) and a frozen one; three
    steps with a changing rate and a 1/2 gradient scale, with (bf16) and without (fp32) a shadow"""
    gen = torch.Generator().manual_seed(5)
    params = [("a.weight", torch.nn.Parameter(torch.randn(33, 7, generator=gen))),
              ("a.bias", torch.nn.Parameter(torch.randn(33, generator=gen))),
              ("frozen", torch.nn.Parameter(torch.randn(5, 5, generator=gen)))]
    arena = ParamArena(params, ["a.weight", "a.bias"], dtype, torch.device(DEV))
    n = arena.n_grad
    assert n == 320 and (arena.shadow is not None) == (dtype == torch.bfloat16)
    live = np.zeros(n, bool)
    for name in ("a.weight", "a.bias"):
        o = arena.offsets[name]
        live[o:o + dict(params)[name].numel()] = True
    assert (~live).sum() == 25 + 31
    opt = ArenaAdamW(arena, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, max_grad_norm=1.0)
    frozen = arena.data[n:].cpu().clone()
    case = dict(lr=None, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.01, step0=1, max_norm=1.0, grad_scale=0.5)
    mp, mm, mv = arena.data[:n].cpu().numpy().copy(), np.zeros(n, F), np.zeros(n, F)
    for k, (lr, scale) in enumerate(((1e-3, 3.0), (4e-6, 1e-3), (0.0, 1e-2))):  # clips, does not, lr = 0
        g = np.where(live, np.random.default_rng(40 + k).standard_normal(n) * scale, 0.0).astype(F)
        arena.grad[:n].copy_(torch.from_numpy(g))
        opt.step(lr=lr, grad_scale=0.5)
        pair = opt.norm_out.cpu().numpy()
        total, factor = OC.reference_clip(g, 1.0, 0.5)
        assert abs(float(pair[0]) - total) <= OC.norm_tolerance(n) * total
        assert bits(pair[1]) == bits(OC.model_clip_factor(pair[0], 1.0, 0.5)) and (pair[1] < 0.5) == (k == 0)
        case.update(lr=lr, grad_fn=lambda _k, _g=g: _g)
        _, _, mp, mm, mv = OC.model_step(case, k, mp, mm, mv, clip_pair=(pair[0], pair[1]))
        assert opt.step_count == k + 1
        assert same_bits(arena.data[:n].cpu().numpy(), mp) and same_bits(arena.exp_avg[:n].cpu().numpy(), mm)
        assert same_bits(arena.exp_avg_sq[:n].cpu().numpy(), mv)
        for a in (mp, mm, mv):
            assert (bits(a)[~live] == 0).all()  # the padding stays +0
        if arena.shadow is not None:
            got = arena.shadow[:n].cpu().view(torch.int16).numpy().view(np.uint16)
            assert (got == OC.bf16_bits(mp)).all()
            assert torch.equal(arena.shadow[:n], arena.data[:n].to(torch.bfloat16))
        assert torch.equal(arena.data[n:].cpu(), frozen)
    for name, p in params[:2]:  # the parameters are views of the arena: they show the update
        o = arena.offsets[name]
        assert same_bits(p.data.cpu().numpy().reshape(-1), mp[o:o + p.numel()])
