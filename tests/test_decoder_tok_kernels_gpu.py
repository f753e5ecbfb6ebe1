"""Kernel-level pins of csrc/decoder_tok.hip: s2h_dec_self, s2h_dec_post_a, s2h_dec_post_b and s2h_dec_final
called directly with plain tensors, every stored output checked against the float64 model of the stage that
produced it (dec_tok_cases.py: the shapes, operand classes, stage models and tolerances, and in
test_decoder_tok_host.py the proof that those checks catch the defects they are there for).

Every input lies inside a NaN-filled buffer, every output inside a -9-filled one with 16 more rows of -9
past row R and guards of 16 / 24 / 32 elements around it: no output may hold NaN, and nothing outside the
R rows of a slot may change.  Both weight-prefetch schedules (s2h_dec_sched 0 / 1) run on every case and
must agree bit for bit on every slot, statistic and lse.  The shapes a launch must refuse are refused with
every output untouched.  The step-level tests of these kernels stay in test_decoder_tok_gpu.py."""
import numpy as np
import pytest
import torch

import dec_tok_cases as dc

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
TAIL_ROWS = 16

# the C argument order of each entry point (include/sam2hip.h); a name is an input or an output slot
ARGS = {
    "self": ["R", "T", "flag", "scale", "x", "pe", "wq", "bq", "wk", "bk", "wv", "bv", "wo", "bo", "g1", "b1", "eps", "wqc",
             "bqc", "qa", "qs", "ks", "vs", "os", "lse", "y1", "x1", "mean1", "rstd1", "qt", "qq"],
    "post_a": ["R", "T", "ot", "x1", "wo", "bo", "g2", "b2", "eps", "y2", "x2", "mean2", "rstd2"],
    "post_b": ["R", "T", "flag", "y3", "pe", "g3", "b3", "eps", "wki", "bki", "wvi", "bvi", "wqf", "bqf", "x3", "mean3",
               "rstd3", "q2", "kio", "vio", "qfa", "qqf"],
    "final": ["R", "T", "of", "x3", "wo", "bo", "g", "b", "eps", "y", "hs", "mean", "rstd"],
}
ENTRY = {k: "s2h_dec_" + k for k in dc.KERNELS}


def _lib():
    from sam2_video.kernels import _lib as L
    return L


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _is_f32_input(name):
    return name[0] in "bg"  # biases, gamma, beta; activations and weights are bf16


class Launch:
    """the device buffers of one case: its inputs uploaded once, fresh outputs for every run"""

    def __init__(self, c):
        self.c, self.inp = c, dc.build(c)
        ins = {n: v for n, v in self.inp.items() if isinstance(v, np.ndarray)}
        self.in_bf, self.in_f = dc.Arena(NAN), dc.Arena(NAN)
        for n, v in ins.items():
            (self.in_f if _is_f32_input(n) else self.in_bf).add(n, v.shape, tail=8)
        self.d_in_bf = torch.from_numpy(self.in_bf.host(ins)).to(torch.bfloat16).to(DEV)
        self.d_in_f = torch.from_numpy(self.in_f.host(ins)).to(DEV)
        self.out_bf, self.out_f = dc.Arena(dc.SENT), dc.Arena(dc.SENT)
        for n, kind in dc.present(c):
            shape = dc.slot_shape(c, kind)
            if kind in (256, 128):
                self.out_bf.add(n, shape, tail=TAIL_ROWS * kind)
            else:
                self.out_f.add(n, shape, tail=TAIL_ROWS * dc.HEADS)

    def ptr(self, name, outs):
        if name in self.in_bf.slots:
            return self.d_in_bf.data_ptr() + 2 * self.in_bf.offset(name)
        if name in self.in_f.slots:
            return self.d_in_f.data_ptr() + 4 * self.in_f.offset(name)
        if name in self.out_bf.slots:
            return outs[0].data_ptr() + 2 * self.out_bf.offset(name)
        if name in self.out_f.slots:
            return outs[1].data_ptr() + 4 * self.out_f.offset(name)
        return None  # a slot this case does not have (qa with skip; qfa / qqf / wqf / bqf without final_q)

    def run(self, **override):
        """one launch into fresh output buffers -> (bf16 flat, fp32 flat) on the device.  override: R, T, flag, or
        a pointer name -> None"""
        c = self.c
        outs = (torch.full((self.out_bf.n,), dc.SENT, dtype=torch.bfloat16, device=DEV),
                torch.full((self.out_f.n,), dc.SENT, dtype=torch.float32, device=DEV))
        scalars = {"R": c.T * c.objects, "T": c.T, "flag": c.flag, "scale": self.inp.get("scale"), "eps": self.inp["eps"]}
        args = []
        for name in ARGS[c.kernel]:
            if name in override:
                args.append(override[name])
            elif name in scalars:
                args.append(scalars[name])
            elif c.kernel == "post_b" and not c.flag and name in ("wqf", "bqf"):
                args.append(None)
            else:
                args.append(self.ptr(name, outs))
        self.outs = outs
        _lib().call(ENTRY[c.kernel], *args, _stream())
        return outs

    def read(self, outs):
        """-> ({slot: fp32 array}, the failures of the buffer checks)"""
        got, fails = {}, []
        for arena, t in ((self.out_bf, outs[0]), (self.out_f, outs[1])):
            g, ok = arena.read(t.float().cpu().numpy())
            got.update(g)
            if not ok:
                fails.append("a guard or a row past R was written")
        for n, v in got.items():
            if np.isnan(v).any():
                fails.append(f"{n}: {int(np.isnan(v).sum())} NaN")
        return got, fails


@pytest.fixture(scope="module")
def sched():
    """both schedules inside, the previous setting restored afterwards"""
    lib = _lib().lib()
    prev = lib.s2h_dec_sched(-1)
    try:
        yield lib.s2h_dec_sched
    finally:
        lib.s2h_dec_sched(prev)


@pytest.mark.parametrize("kernel", dc.KERNELS)
def test_every_stage_against_float64(sched, kernel):
    """every shape, class and flag: each stored output within its stage's tolerance of float64 (equality for the
    adds and the exact class's integer slots), no NaN, guards intact, and the two schedules bit-identical"""
    fails, top = [], {}
    for c in dc.cases(kernel):
        L = Launch(c)
        sched(1)
        a = L.run()
        sched(0)
        b = L.run()
        what = dc.case_id(c)
        if not (torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])):
            fails.append(f"{what}: the two schedules differ")
        got, bad = L.read(a)
        fails += [f"{what}: {m}" for m in bad]
        for slot, (ratio, row) in dc.worst(dc.check(c, L.inp, got)).items():
            if ratio > top.get(slot, (-1.0, ""))[0]:
                top[slot] = (ratio, what)
            if not ratio <= 1:
                fails.append(f"{what}: {slot}[{row}] error / tolerance {ratio:.3g}")
    for slot, (ratio, what) in top.items():
        print(f"{kernel} {slot:6s} worst error / tolerance {ratio:.3f}  {what}")
    assert not fails, f"{len(fails)} failure(s):\n" + "\n".join(fails[:60])


def _refused(L, what, fails, **override):
    try:
        L.run(**override)
        fails.append(f"{what}: launched")
    except _lib().HipKernelError:
        pass
    torch.cuda.synchronize()
    if not all(bool((t == dc.SENT).all()) for t in L.outs):
        fails.append(f"{what}: an output was written")


@pytest.mark.parametrize("kernel", dc.KERNELS)
def test_refusals(sched, kernel):
    """T = 0, T = 17, R not a multiple of T, R = 0 (and final_q = 1 with a null qfa, qqf or wqf): HipKernelError
    from every entry point on both schedules, and every output buffer still all sentinel.  The buffers are
    those of a valid 8 x 13 case, so no refused shape reaches past them."""
    c = dc.find(kernel, 8, 13, "real", 1 if kernel == "post_b" else 0)
    assert c in dc.cases(kernel)
    L, fails = Launch(c), []
    for mode in (1, 0):
        sched(mode)
        _refused(L, f"sched {mode} T = 0", fails, R=8, T=0)
        _refused(L, f"sched {mode} T = 17", fails, R=34, T=17)
        _refused(L, f"sched {mode} R = 20, T = 8", fails, R=20, T=8)
        _refused(L, f"sched {mode} R = 0", fails, R=0, T=8)
        _refused(L, f"sched {mode} R = -8", fails, R=-8, T=8)
        if kernel == "post_b":
            for name in ("qfa", "qqf", "wqf"):
                _refused(L, f"sched {mode} final_q with a null {name}", fails, **{name: None})
    assert not fails, "\n".join(fails)
