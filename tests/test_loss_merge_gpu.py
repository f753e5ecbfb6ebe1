"""csrc/loss.hip -- the fused focal + Dice + IoU-L1 loss, the BCE category loss and the object-to-category
merge in front of them -- on the rows of loss_cases.py (gated-off objects at -1024, logits saturated at +-40
and +-90, zeros of both signs, target bytes 2 and 255, an empty target) against the float64 models there,
through every kernel the shape and the alignment select: P 3 and 4099 (scalar), 4100 (vector, three
workgroups, the last nearly empty), 8192 (exact multiple), and at P 4100 a row stride of P + 4 (vector),
of P + 1 and a base 4 bytes off (both scalar); statistics with the deterministic partial-row reduction and
with float atomics.  The padding of strided rows holds a sentinel: NaN logits and set targets that the
statistics would show if read, a value in the gradient buffers that must survive.

The assertions and their tolerances are loss_cases.py's (check_*), against float64 and never against another
kernel path: integer statistics and selections exact, sums 2e-5 |ref| + 1e-6 per row, gradients 2e-5 of the
row maximum + 1e-12.  test_loss_merge_host.py proves that each can fail by more than 10x.

Not asserted: merge weights of a category whose every pixel lies in roughly (-104, -87), where fp32 torch
keeps a denormal sigmoid mass and the hardware exponential may flush it (no case here sits in that band).

Observed maxima on an MI355X over all cases, as error / tolerance (the libm fp32 model of loss_cases.py gives
sums 0.005, gradients 0.08, so the hardware exp / log / rcp add nothing that shows):
  mask_stats focal / sigma / sigma.t sums   0.0074 / 0.0061 / 0.0054   (1.5e-7 relative)
  mask_loss_finalize losses / coefficients  0.012 / 0.0095             (two frames 0.012)
  mask_loss_bwd dx / dious                  0.082 / 0.0022             (1.6e-6 of the row maximum)
  bce row sums / loss / coef / dx           0.0083 / 0.0066 / 0.0022 / 0.0083
  group_wavg y / ds / dw / logit gradient   0.0050 / 0.0029 / 0.019 / 0.0027
  modules: losses / dx / dious              0.0059 / 0.077 / 0.0022;  BCE loss / dx 0.0020 / 0.0067
Every exact assertion (counts, selections, zeros, the gated-off row, identical bits of the fixed-order
reduction) held.  Nothing is above a quarter of its tolerance.
"""
import pytest
import torch

import loss_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (P, row padding, base offset in elements): which kernels the layout selects
LAYOUTS = [(3, 0, 0), (4099, 0, 0), (4100, 0, 0), (8192, 0, 0), (4100, 4, 0), (4100, 1, 0), (4100, 0, 1)]
LAYOUT_IDS = ["3-scalar", "4099-scalar", "4100-vector", "8192-vector", "4100-ld+4-vector", "4100-ld+1-scalar",
              "4100-base+4B-scalar"]
PS = [3, 4099, 4100, 8192]
GRAD_FILL = 7.25


def _ops():
    from sam2_video.kernels import ops
    return ops


@pytest.fixture(scope="module", autouse=True)
def _workspace():
    """the deterministic-reduction workspace registered, so that the reduction each case runs is the one it
    names and not whatever an earlier module left"""
    ops = _ops()
    ops.wgrad_workspace(DEV)
    ops._det_workspace_mode(True)
    yield
    ops._det_workspace_mode(True)


class Hip:
    """the check_* backend over the HIP kernels: rows placed at the layout's stride and base inside
    sentinel-filled buffers; det = the statistics' reduction (partial rows in fixed order / float atomics)"""

    def __init__(self, pad=0, off=0, det=True):
        self.pad, self.off, self.det = pad, off, det
        self.ops = _ops()

    def _place(self, src, fill, dtype=None):
        N, P = src.shape
        ld = P + self.pad
        buf = torch.full((N * ld + 8,), fill, dtype=dtype or src.dtype, device=DEV)
        view = buf[self.off:self.off + N * ld].view(N, ld)[:, :P]
        view.copy_(src)
        return buf, view

    def _padding_kept(self, buf, view, fill):
        N, P = view.shape
        ld = P + self.pad
        inside = torch.zeros_like(buf, dtype=torch.bool)
        inside[self.off:self.off + N * ld].view(N, ld)[:, :P] = True
        assert bool((buf[~inside] == fill).all()), "the kernel wrote outside its rows"

    def _reduced(self, fn):
        ops = self.ops
        try:
            ops._det_workspace_mode(self.det)
            a = fn().clone()
            if self.det:
                assert torch.equal(a.view(torch.int32), fn().view(torch.int32)), "the fixed-order reduction moved"
        finally:
            ops._det_workspace_mode(True)
        return a.cpu()

    def stats(self, x, t, inv_temp=1.0):
        _, xv = self._place(x, float("nan"))
        tv = None if t is None else self._place(t, 255)[1]
        return self._reduced(lambda: self.ops.mask_stats(xv, tv, inv_temp))

    def finalize(self, stats, pred_iou, valid, P, weights, gscale, losses):
        losses = losses.to(DEV)
        coef = torch.full((stats.shape[0], 4), float("nan"), device=DEV)
        self.ops.mask_loss_finalize(stats.to(DEV), pred_iou.to(DEV).contiguous(), None if valid is None else valid.to(DEV),
                                    P, weights, gscale, losses, coef)
        return losses.cpu(), coef.cpu()

    def bwd(self, x, t, coef, inv_temp, gtot):
        _, xv = self._place(x, float("nan"))
        _, tv = self._place(t, 255)
        buf, dx = self._place(torch.full(x.shape, float("nan")), GRAD_FILL)
        dious = torch.full((x.shape[0], 1), float("nan"), device=DEV)
        self.ops.mask_loss_bwd(xv, tv, coef.to(DEV), inv_temp, dx, gtot=None if gtot is None else gtot.to(DEV), dious=dious)
        self._padding_kept(buf, dx, GRAD_FILL)
        return dx.cpu(), dious.cpu()

    def _groups(self, groups):
        from sam2_video.utils.masks import CategoryGroups
        return CategoryGroups(groups.obj_to_cat, groups.ncat, DEV)

    def gmax(self, x, groups):
        g = self._groups(groups)
        _, xv = self._place(x, float("nan"))
        buf, y = self._place(torch.full((groups.ncat, x.shape[1]), float("nan")), GRAD_FILL)
        arg = torch.full((groups.ncat, x.shape[1]), -7, dtype=torch.int32, device=DEV)
        self.ops.group_max(xv, g.cat_off, g.cat_obj, g.ncat, y, arg)
        self._padding_kept(buf, y, GRAD_FILL)
        return y.cpu(), arg.cpu()

    def gmax_bwd(self, dy, arg, groups):
        g = self._groups(groups)
        _, dyv = self._place(dy, float("nan"))
        buf, dx = self._place(torch.full((len(groups.obj_to_cat), dy.shape[1]), float("nan")), GRAD_FILL)
        self.ops.group_max_bwd(dyv, g.obj_cat, arg.to(DEV), dx)
        self._padding_kept(buf, dx, GRAD_FILL)
        return dx.cpu()

    def wavg(self, s, stats, groups):
        g = self._groups(groups)
        out = torch.full((groups.ncat, s.shape[1]), float("nan"), device=DEV)
        return self.ops.group_wavg(s.to(DEV), stats.to(DEV), g.cat_off, g.cat_obj, g.ncat, out).cpu()

    def wavg_bwd(self, s, y, dy, stats, groups):
        g = self._groups(groups)
        ds = torch.full(s.shape, float("nan"), device=DEV)
        dw = torch.full((s.shape[0],), float("nan"), device=DEV)
        self.ops.group_wavg_bwd(s.to(DEV), y.to(DEV), dy.to(DEV), stats.to(DEV), g.obj_cat, g.cat_off, ds, dw)
        return ds.cpu(), dw.cpu()

    def sig_axpy(self, hr, coef, dx):
        _, xv = self._place(hr, float("nan"))
        buf, dxv = self._place(dx, GRAD_FILL)
        self.ops.sigmoid_grad_axpy(xv, coef.to(DEV), dxv)
        self._padding_kept(buf, dxv, GRAD_FILL)
        return dxv.cpu()

    # the BCE category loss
    def bce_stats(self, x, t, inv_temp, pw):
        _, xv = self._place(x, float("nan"))
        _, tv = self._place(t, 255)
        pwd = None if pw is None else pw.to(DEV)
        return self._reduced(lambda: self.ops.bce_stats(xv, tv, inv_temp, pwd))

    def bce_finalize(self, stats, P, reduction, frame_scale, losses):
        losses = losses.to(DEV)
        coef = torch.full((stats.shape[0],), float("nan"), device=DEV)
        self.ops.bce_finalize(stats.to(DEV), P, reduction, frame_scale, losses, coef)
        return losses.cpu(), coef.cpu()

    def bce_bwd(self, x, t, inv_temp, pw, coef, gtot):
        _, xv = self._place(x, float("nan"))
        _, tv = self._place(t, 255)
        buf, dx = self._place(torch.full(x.shape, float("nan")), GRAD_FILL)
        self.ops.bce_bwd(xv, tv, inv_temp, None if pw is None else pw.to(DEV), coef.to(DEV), dx,
                         gtot=None if gtot is None else gtot.to(DEV))
        self._padding_kept(buf, dx, GRAD_FILL)
        return dx.cpu()


def _hold(ratios):
    worst = max(ratios, key=ratios.get)
    print("worst %.3g (%s)" % (ratios[worst], worst), {k: float("%.3g" % v) for k, v in ratios.items() if v > 0})
    assert not C.failed(ratios), C.failed(ratios)


# ------------------------------------------------------------------ the fused mask loss
@pytest.mark.parametrize("inv_temp", C.INV_TEMPS, ids=["T1", "T0.7"])
@pytest.mark.parametrize("det", [True, False], ids=["fixed-order", "atomics"])
@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
def test_mask_stats(layout, det, inv_temp):
    """columns 2, 4, 5 exact, columns 0, 1, 3 per row; NaN logits and set targets in the padding stay unread"""
    P, pad, off = layout
    _hold(C.check_mask_stats(Hip(pad, off, det), P, inv_temp))


@pytest.mark.parametrize("det", [True, False], ids=["fixed-order", "atomics"])
@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
def test_mask_stats_without_target(layout, det):
    """tgt = NULL (the merge weights): every target 0"""
    P, pad, off = layout
    _hold(C.check_mask_stats(Hip(pad, off, det), P, 1.0, with_tgt=False))


@pytest.mark.parametrize("inv_temp", C.INV_TEMPS, ids=["T1", "T0.7"])
@pytest.mark.parametrize("P", PS)
def test_mask_loss_finalize(P, inv_temp):
    """all four losses and coefficient columns: explicit and derived valid flags (the same bits when they
    agree), a flag on the row without target pixels (it counts), two frames into one buffer, gscale 0.5,
    pred_iou equal to / above / below the actual IoU (sign 0 / +1 / -1), a gated-off row with an empty union.
    A frame with no valid row leaves the losses as they were and writes zero coefficients, all finite -- the
    project being rebuilt raises "No valid masks" there instead."""
    _hold(C.check_finalize(Hip(), P, inv_temp))


@pytest.mark.parametrize("gs", [0.37, None], ids=["gtot0.37", "no-gtot"])
@pytest.mark.parametrize("inv_temp", C.INV_TEMPS, ids=["T1", "T0.7"])
@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
def test_mask_loss_bwd(layout, inv_temp, gs):
    """dx and dious against float64 autograd (gscale 0.5 in the coefficients); the invalid row zeros; the
    gated-off row exactly -0.25 c0 inv_temp gs on set pixels and 0 elsewhere; the padding of dx untouched"""
    P, pad, off = layout
    _hold(C.check_mask_bwd(Hip(pad, off), P, inv_temp, gs))


def test_mask_loss_bwd_refuses_a_null_target():
    """both kernels read the targets of every row with a non-zero coefficient: tgt = NULL is
    hipErrorInvalidValue before any launch, and dx stays as it was"""
    from sam2_video.kernels._lib import HipKernelError, call
    ops = _ops()
    for P in (4099, 4100):
        x = torch.randn(2, P, device=DEV)
        coef = torch.zeros(2, 4, device=DEV)  # nothing would read a target even without the guard
        dx = torch.full((2, P), GRAD_FILL, device=DEV)
        with pytest.raises(HipKernelError, match="hipError 1$"):
            call("s2h_mask_loss_bwd", 2, P, x.data_ptr(), P, None, 0, 1.0, coef.data_ptr(), dx.data_ptr(), P, None, None,
                 ops.stream())
        torch.cuda.synchronize()
        assert bool((dx == GRAD_FILL).all())


# ------------------------------------------------------------------ the BCE category loss
PW = [0.5, 2.0, 1.0, 3.0, 0.25, 1.5, 4.0, 1.0]


def check_bce(be, P, pw, reduction, inv_temp):
    x, t = C.make_rows(P)
    it = C.f32(inv_temp)
    pwt = None if pw is None else torch.tensor(pw)
    out = {}
    stats = be.bce_stats(x, t, inv_temp, pwt)
    out["bce.rows"] = C.sum_ratio(stats[:, 0], C.bce_rows64(x, t, pwt, it).sum(1))
    out["bce.tsum"] = C.exact(stats[:, 1].double(), (t != 0).sum(1).double())
    before = torch.tensor([0.25])
    losses, coef = be.bce_finalize(stats, P, reduction, 0.5, before.clone())
    out["bce.loss"] = C.sum_ratio(losses, 0.25 + C.bce64(x, t, pwt, it, reduction, C.f32(0.5)).view(1))
    has = (t != 0).sum(1) > 0
    cref = has.double() * (0.5 / (int(has.sum()) * P if reduction == 0 else 1.0))
    out["bce.coef"] = C.rel_ratio(coef, cref)
    for gs in (0.37, None):
        dx = be.bce_bwd(x, t, inv_temp, pwt, coef, None if gs is None else torch.tensor([gs]))
        ref = C.bce_grad64(x, t, pwt, it, reduction, 0.5, 1.0 if gs is None else C.f32(gs))
        out["bce.dx" + ("" if gs else ".no_gtot")] = C.grad_ratio(dx, ref)
        out["bce.invalid_row_zero"] = max(out.get("bce.invalid_row_zero", 0.0), C.exact(dx[C.ROW_EMPTY], torch.zeros(P)))
    # no row with target pixels: the mean of nothing is NaN, as torch's; the sum adds 0; no gradient
    empty = torch.zeros_like(t)
    s0 = be.bce_stats(x, empty, inv_temp, pwt)
    l0, c0 = be.bce_finalize(s0, P, reduction, 0.5, before.clone())
    out["bce.none_valid.loss"] = C.exact(l0, torch.tensor([float("nan")]) if reduction == 0 else before)
    out["bce.none_valid.coef"] = C.exact(c0, torch.zeros(8))
    out["bce.none_valid.dx"] = C.exact(be.bce_bwd(x, empty, inv_temp, pwt, c0, None), torch.zeros(8, P))
    return out


@pytest.mark.parametrize("reduction", [0, 1], ids=["mean", "sum"])
@pytest.mark.parametrize("pw", [None, PW], ids=["no-pw", "pw"])
@pytest.mark.parametrize("layout,det", [((3, 0, 0), True), ((4099, 0, 0), False), ((4100, 0, 0), True), ((8192, 0, 0), False),
                                        ((4100, 1, 1), True)], ids=["3", "4099-atomics", "4100", "8192-atomics", "4100-ld+1-base+4B"])
def test_bce_category_kernels(layout, det, pw, reduction):
    """bce_stats / bce_finalize / bce_bwd on the same rows at temperature 0.7"""
    P, pad, off = layout
    _hold(check_bce(Hip(pad, off, det), P, pw, reduction, 1.0 / 0.7))


# ------------------------------------------------------------------ the category merge
@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
def test_group_max(layout):
    """categories of 0, 1, 2 and 3 objects, y and dx strided: values bit for bit, arg on every column but the
    +0.0 / -0.0 ties, NaN positions, the empty category y = 0 / arg = -1; the backward hands every dy to
    exactly one object of its category"""
    P, pad, off = layout
    _hold(C.check_group_max(Hip(pad, off), P))


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("layout", LAYOUTS[:4] + LAYOUTS[5:6], ids=LAYOUT_IDS[:4] + LAYOUT_IDS[5:6])
def test_group_wavg_and_weight_gradient(layout, K):
    """weights from mask_stats(hr, None): a weighted category, a live object beside a gated-off one, a
    category of gated-off objects only (the plain mean: dx = g / cnt, dw = 0, logit gradient untouched), an
    empty one; sigmoid_grad_axpy adds into a non-zero dx and skips the rows whose coefficient is 0"""
    P, pad, off = layout
    _hold(C.check_wavg(Hip(pad, off), P, K))


# ------------------------------------------------------------------ the loss modules
def _clip():
    H = 64
    frames = [C.make_rows(H * H, seed) for seed in (0, 1)]
    x = torch.stack([f[0] for f in frames]).view(2, 8, 1, H, H)
    t = torch.stack([f[1] for f in frames]).view(2, 8, H, H)
    return x, t, torch.stack([C.pred_ious(H * H, seed) for seed in (0, 1)]).view(2, 8, 1)


def test_multistep_loss_module_on_a_two_frame_clip():
    """MultiStepMultiMasksAndIous at temperature 0.7 (derived valid flags, both frames into one buffer): the
    four losses and d total / d logits, d total / d pred_iou against float64"""
    from sam2_video.model.losses import MultiStepMultiMasksAndIous
    x, t, ious = _clip()
    xd = x.to(DEV).requires_grad_(True)
    iod = ious.to(DEV).requires_grad_(True)
    crit = MultiStepMultiMasksAndIous({"loss_mask": 20.0, "loss_dice": 1.0, "loss_iou": 1.0}, iou_use_l1_loss=True,
                                      logit_temperature=0.7)
    outs = [{"multistep_pred_multimasks_high_res": [xd[f]], "multistep_pred_ious": [iod[f]]} for f in range(2)]
    got = crit(outs, t.to(DEV))
    got["total_loss"].backward()
    it = 1.0 / 0.7
    ref = sum(C.frame64(x[f].view(8, -1), t[f].view(8, -1), ious[f].view(8), None, C.WEIGHTS, it) for f in range(2))
    terms = torch.stack([got[k].detach() for k in ("loss_mask", "loss_dice", "loss_iou", "total_loss")]).cpu()
    out = {"module.losses": C.sum_ratio(terms, ref)}
    for f in range(2):
        rx, ri = C.frame_grads64(x[f].view(8, -1), t[f].view(8, -1), ious[f].view(8), None, C.WEIGHTS, it)
        out["module.dx.frame%d" % f] = C.grad_ratio(xd.grad[f].view(8, -1).cpu(), rx)
        out["module.dious.frame%d" % f] = C.rel_ratio(iod.grad[f].view(8).cpu(), ri)
    _hold(out)


def test_bce_loss_module_on_a_two_frame_clip():
    """BCECategoryLoss with pos_weight at temperature 0.7, the mean over the rows with target pixels averaged
    over the frames: loss and d loss / d logits against float64"""
    from sam2_video.model.losses import BCECategoryLoss
    x, t, _ = _clip()
    xd = x.to(DEV).requires_grad_(True)
    crit = BCECategoryLoss(pos_weight=PW, reduction="mean", logit_temperature=0.7)
    got = crit([{"pred_masks_high_res": xd[f]} for f in range(2)], t.to(DEV))
    got["total_loss"].backward()
    it, pwt = 1.0 / 0.7, torch.tensor(PW)
    ref = sum(C.bce64(x[f].view(8, -1), t[f].view(8, -1), pwt, it, 0, 0.5) for f in range(2))
    out = {"module.bce": C.sum_ratio(got["total_loss"].detach().view(1).cpu(), ref.view(1))}
    for f in range(2):
        rx = C.bce_grad64(x[f].view(8, -1), t[f].view(8, -1), pwt, it, 0, 0.5)
        out["module.bce.dx.frame%d" % f] = C.grad_ratio(xd.grad[f].view(8, -1).cpu(), rx)
    _hold(out)
