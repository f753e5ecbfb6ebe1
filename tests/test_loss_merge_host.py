"""The cases of loss_cases.py can fail, proven on the CPU alone: the float64 models agree with torch's own
binary_cross_entropy_with_logits, sigmoid, max(dim) and autograd in float64 on the regime rows; the fp32
model of the kernels' arithmetic (csrc/loss.hip: one exponential per pixel) holds every assertion that
test_loss_merge_gpu.py makes, with room; and each switchable defect of that model breaks a named assertion by
more than 10x its tolerance (exactly, for the integer and selection assertions).  The inputs are checked to be
what the assertions need: a gated-off row of sigmoid mass exactly 0, x == 0 under a set target, saturated
rows whose 1 + e rounds to 1."""
import math

import pytest
import torch
import torch.nn.functional as F

import loss_cases as C

PS = [3, 4099, 4100, 8192]
F64 = torch.float64


def _clean():
    return C.KernelModel()


def _all_checks(be, P):
    out = {}
    for it in C.INV_TEMPS:
        tag = "T%.2f." % (1 / it)
        for name, r in C.check_mask_stats(be, P, it).items():
            out[tag + name] = r
        for name, r in C.check_finalize(be, P, it).items():
            out[tag + name] = r
        for gs in (0.37, None):
            for name, r in C.check_mask_bwd(be, P, it, gs).items():
                out[tag + ("gs." if gs else "nogs.") + name] = r
    for name, r in C.check_mask_stats(be, P, 1.0, with_tgt=False).items():
        out["notgt." + name] = r
    out.update(C.check_group_max(be, P))
    for K in (1, 3):
        for name, r in C.check_wavg(be, P, K).items():
            out["K%d." % K + name] = r
    return out


# ------------------------------------------------------------------ the inputs are what the assertions need
@pytest.mark.parametrize("P", PS)
def test_rows_hold_the_regimes(P):
    x, t = C.make_rows(P)
    on = t != 0
    assert x.dtype == torch.float32 and t.dtype == torch.uint8 and x.shape == t.shape == (8, P)
    assert set(t[on].tolist()) <= set(C.SET_BYTES) and (P < 64 or set(t[on].tolist()) == set(C.SET_BYTES))
    assert not on[C.ROW_EMPTY].any() and all(on[r].any() for r in range(8) if r != C.ROW_EMPTY)
    # the gated-off row: sigmoid mass exactly 0 in fp32 and in float64, at both temperatures
    for it in C.INV_TEMPS:
        assert float(torch.sigmoid(x[C.ROW_GATED] * C.f32(it)).sum()) == 0.0
        assert float(torch.sigmoid(x[C.ROW_GATED].double() * C.f32(it)).sum()) == 0.0
    assert float(C.KernelModel().stats(x, None)[C.ROW_GATED, 1]) == 0.0
    # x == 0 under a set target: background for the IoU count
    assert bool(((x[C.ROW_ZEROS] == 0) & on[C.ROW_ZEROS]).any())
    # the saturated rows: 1 + e == 1 in fp32
    for r in (C.ROW_RIGHT, C.ROW_WRONG):
        assert bool((1.0 + torch.exp(-x[r].abs()) == 1.0).all())
    assert float(x[C.ROW_WIDE].abs().max()) <= 90.0 and (P < 64 or float(x[C.ROW_WIDE].abs().max()) > 80.0)


@pytest.mark.parametrize("P", PS)
def test_merge_categories_hold_the_branches(P):
    hr = C.make_objects(P)
    w32 = torch.sigmoid(hr).sum(1)
    w64 = torch.sigmoid(hr.double()).sum(1)
    m = C.GROUPS.members
    assert [len(g) for g in m] == [0, 1, 2, 3, 2]
    assert float(w32[m[C.CAT_GATED]].sum()) == 0.0 and float(w64[m[C.CAT_GATED]].sum()) == 0.0
    assert min(C.weighted_masses(P)) >= 1.0 and len(C.weighted_masses(P)) == 3
    gated_in_mixed = [o for o in m[C.CAT_MIXED] if float(w64[o]) == 0.0]
    assert len(gated_in_mixed) == 1
    # no category sits in the band where fp32 keeps a denormal mass the hardware exponential may flush
    for g in m:
        for o in g:
            assert not bool(((hr[o] > -104) & (hr[o] < -87)).all())
    x = C.make_max_objects(P)
    ties = C.zero_tie_columns(x, C.GROUPS)
    assert int(ties.sum()) == min(P, 2) and bool(ties[C.CAT_WEIGHTED, 0])
    if P > 5:
        assert bool(torch.isnan(x[:, 2:4]).any()) and bool((x[m[C.CAT_WEIGHTED], 4] == -math.inf).all())


# ------------------------------------------------------------------ the float64 models against torch
@pytest.mark.parametrize("it", C.INV_TEMPS)
@pytest.mark.parametrize("P", [3, 4100])
def test_float64_loss_models_agree_with_torch(P, it):
    x, t = C.make_rows(P)
    xv = (x.double() * it).requires_grad_(True)
    tb = (t != 0).double()
    ce = F.binary_cross_entropy_with_logits(xv, tb, reduction="none")
    # torch adds softplus(-|x|) to |x| before it takes |x| away again: an ulp of |x| <= 1463, absolute
    assert torch.allclose(C.ce64(xv, tb), ce, rtol=1e-13, atol=3e-13)
    s = torch.sigmoid(xv)
    focal = (0.25 * tb + 0.75 * (1 - tb)) * ce * (1 - (s * tb + (1 - s) * (1 - tb))) ** 2
    st = C.stats64(x, t, it)
    assert torch.allclose(st[:, 0], focal.sum(1).detach(), rtol=1e-12)
    assert torch.allclose(st[:, 1], s.sum(1).detach(), rtol=1e-13)
    assert torch.equal(st[:, 2], tb.sum(1)) and torch.equal(st[:, 4], ((xv > 0) & (tb > 0)).sum(1).double())
    # the frame loss and its gradients: torch's formulas under autograd, on the valid rows only
    ious = C.pred_ious(P).double().requires_grad_(True)
    v = tb.sum(1) > 0
    nv = int(v.sum())
    lm = focal.mean(1)[v].sum() / nv
    ld = (1 - (2 * (s * tb).sum(1) + 1) / (s.sum(1) + tb.sum(1) + 1))[v].sum() / nv
    li = F.l1_loss(ious, st[:, 4] / st[:, 5].clamp(min=1.0), reduction="none")[v].sum() / nv
    total = 20 * lm + ld + li
    got = C.frame64(x, t, C.pred_ious(P), None, C.WEIGHTS, it)
    assert torch.allclose(got, torch.stack([lm, ld, li, total]).detach(), rtol=1e-12)
    gx, gi = torch.autograd.grad(total, [xv, ious], retain_graph=True)
    rx, ri = C.frame_grads64(x, t, C.pred_ious(P), None, C.WEIGHTS, it, 0.37)
    assert C.grad_ratio(rx, gx * it * 0.37) < 1e-6 and torch.allclose(ri, gi * 0.37, rtol=1e-12)
    # the closed-form coefficients reproduce that gradient: dx = it (c0 dfocal/dx - (c1 t - c2) sigma')
    c = C.coef64(st, C.pred_ious(P), None, P)
    (dfocal,) = torch.autograd.grad(focal.sum(), [xv])
    dx = it * (c[:, 0:1] * dfocal - (c[:, 1:2] * tb - c[:, 2:3]) * (s * (1 - s)).detach())
    assert C.grad_ratio(dx, rx / 0.37) < 1e-6 and torch.allclose(c[:, 3], ri / 0.37, rtol=1e-12)
    assert bool((c[C.ROW_EMPTY] == 0).all())
    # no valid row: zeros (the project being rebuilt raises there)
    none = torch.zeros(8, dtype=torch.int32)
    assert bool((C.frame64(x, t, C.pred_ious(P), none) == 0).all())
    assert bool((C.frame_grads64(x, t, C.pred_ious(P), none)[0] == 0).all())


@pytest.mark.parametrize("reduction", [0, 1])
@pytest.mark.parametrize("pw", [None, [0.5, 2.0, 1.0, 3.0, 0.25, 1.5, 4.0, 1.0]])
def test_float64_bce_model_agrees_with_torch(pw, reduction):
    P, it = 4100, 1.0 / 0.7
    x, t = C.make_rows(P)
    pwt = None if pw is None else torch.tensor(pw)
    xd = x.double().requires_grad_(True)
    tb = (t != 0).double()
    v = tb.sum(1) > 0
    ref = F.binary_cross_entropy_with_logits(xd[v] * it, tb[v], pos_weight=None if pw is None else pwt.double().view(-1, 1)[v],
                                             reduction="mean" if reduction == 0 else "sum") / 3
    assert torch.allclose(C.bce64(x, t, pwt, it, reduction, 1 / 3), ref.detach(), rtol=1e-12)
    (g,) = torch.autograd.grad(ref, [xd])
    assert C.grad_ratio(C.bce_grad64(x, t, pwt, it, reduction, 1 / 3, 0.37), g * 0.37) < 1e-6
    empty = torch.zeros_like(t)
    assert math.isnan(float(C.bce64(x, empty, pwt, it, 0))) and float(C.bce64(x, empty, pwt, it, 1)) == 0.0
    assert bool((C.bce_grad64(x, empty, pwt, it, 0) == 0).all())


@pytest.mark.parametrize("P", [3, 4100])
def test_merge_models_agree_with_torch(P):
    x = C.make_max_objects(P)
    y, arg = C.group_max_model(x, C.GROUPS)
    ties = C.zero_tie_columns(x, C.GROUPS)
    for c, objs in enumerate(C.GROUPS.members):
        if not objs:
            assert bool((y[c] == 0).all()) and bool((arg[c] == -1).all())
            continue
        v, i = x[objs].max(dim=0)
        assert C.exact(y[c], v) == 0.0
        ok = ~ties[c] & ~torch.isnan(v)  # torch names an arbitrary NaN holder; the model the first
        assert torch.equal(arg[c][ok].long(), torch.tensor(objs)[i][ok])
        first_nan = torch.isnan(x[objs]).int().argmax(0)
        assert torch.equal(arg[c][torch.isnan(v)].long(), torch.tensor(objs)[first_nan][torch.isnan(v)])
    # the weighted mean and its gradients: the reference's formula under float64 autograd
    hr = C.make_objects(P)
    g = torch.Generator().manual_seed(3)
    s, dy = torch.rand(8, 3, generator=g), torch.randn(5, 3, generator=g)
    ry, rds, rdw, rdhr = C.wavg_grads64(s, hr, dy, C.GROUPS)
    sd, hd = s.double().requires_grad_(True), hr.double().requires_grad_(True)
    w = torch.sigmoid(hd).sum(1)
    rows = []
    for objs in C.GROUPS.members:
        if not objs:
            rows.append(torch.zeros(3, dtype=F64))
        elif bool((w[objs].sum() == 0)):
            rows.append(sd[objs].mean(0))
        else:
            rows.append((sd[objs] * w[objs].view(-1, 1)).sum(0) / w[objs].sum())
    yt = torch.stack(rows)
    gs_, gh_ = torch.autograd.grad((yt * dy.double()).sum(), [sd, hd])
    assert torch.equal(ry, yt.detach()) and torch.equal(rds, gs_) and torch.equal(rdhr, gh_)
    gated = C.GROUPS.members[C.CAT_GATED]
    assert torch.equal(rds[gated], (dy[C.CAT_GATED].double() / 2).expand(2, 3)) and bool((rdw[gated] == 0).all())
    assert bool((rdhr[gated] == 0).all())


# ------------------------------------------------------------------ the fp32 model holds, its defects do not
@pytest.mark.parametrize("P", PS)
def test_clean_fp32_model_holds_every_gpu_assertion(P):
    """measured: sums within 1e-7 relative, gradients within 1.6e-6 of the row maximum -- under a quarter of
    every tolerance"""
    ratios = _all_checks(_clean(), P)
    assert not C.failed(ratios), C.failed(ratios)
    worst = max(ratios, key=ratios.get)
    print("P %d: worst ratio %.3g (%s)" % (P, ratios[worst], worst))
    assert ratios[worst] <= 0.25, (worst, ratios[worst])


# defect -> the assertions (names of _all_checks) at least one of which it must break, at some P
BREAKS = {
    "naive_softplus": ["stats.focal"],
    "pred_ge": ["stats.inter", "stats.union"],
    "no_union_clamp": ["no_target.losses", "no_target.coef"],
    "dice_no_smooth": ["flags.losses", "flags.coef", "no_target.losses"],
    "valid_from_stats": ["flag_on_empty.losses", "flag_on_empty.row_counts", "none_valid.losses_unchanged"],
    "last_max_wins": ["gmax.arg"],
    "zero_mass_weighted": ["wavg.y", "wavg.zero_mass_is_mean"],
    "bwd_no_inv_temp": ["bwd.dx"],
}


@pytest.mark.parametrize("defect", C.DEFECTS)
def test_each_defect_breaks_a_named_assertion_by_10x(defect):
    assert sorted(BREAKS) == sorted(C.DEFECTS)
    hit = {}
    for P in PS:
        ratios = _all_checks(C.KernelModel([defect]), P)
        for name, r in ratios.items():
            if any(name.endswith(want) for want in BREAKS[defect]) and not r < 10.0:
                hit["P%d." % P + name] = r
    print(defect, "breaks", hit)
    assert hit, "no assertion of the GPU file sees the defect %s" % defect
    # ... at every P for all but the temperature defect, which needs inv_temp != 1
    assert all(any(k.startswith("P%d." % P) for k in hit) for P in PS), hit
    if defect == "bwd_no_inv_temp":
        assert all("T0.70" in k for k in hit)
