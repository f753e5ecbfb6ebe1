"""Stochastic weight averaging on the parameter arena (csrc/optim.hip s2h_swa_update / s2h_swa_apply,
kernels/arena.py): the running average bit for bit against CPU torch fp32 `avg + (p - avg) / torch.tensor(n + 1)`
(Lightning's avg_fn, a true division), the transfer into the master and its bf16 shadow, and the arena's buffer
handling.  Sizes: 1, 63, 64, 65 (around one 16-B vector / one wave), 1027 (vector body + scalar tail, several
workgroups), 2^20 + 5 (1025 workgroups) and, once, 8192 * 256 * 4 + 1027: past the 8192-workgroup cap of the
launch, where the grid-stride loop takes a second round."""
import pytest
import torch

from sam2_video.kernels import ops
from sam2_video.kernels.arena import ParamArena

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 1027, 2 ** 20 + 5]


def _values(n, seed):
    """normal-range fp32 of magnitude 1e-6 .. 1e3, both signs"""
    g = torch.Generator().manual_seed(seed)
    mag = torch.pow(10.0, torch.rand(n, generator=g, dtype=torch.float64) * 9.0 - 6.0)
    sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0).double()
    return (mag * sign).float()


def _pair(n, seed):
    avg, p = _values(n, seed), _values(n, seed + 1)
    same = torch.rand(n, generator=torch.Generator().manual_seed(seed + 2)) < 0.25
    p[same] = avg[same]  # elements where p == avg stay exactly where they are
    if n >= 4:
        assert same.any() and not same.all()
    return avg, p


@pytest.mark.parametrize("n_averaged", [0, 1, 2, 7])
@pytest.mark.parametrize("n", SIZES)
def test_swa_update_is_torch_bit_for_bit(n, n_averaged):
    avg, p = _pair(n, 1000 * n_averaged + n % 997)
    want = p.clone() if n_averaged == 0 else avg + (p - avg) / torch.tensor(n_averaged + 1)
    assert want.dtype == torch.float32
    for shift in (0, 1):  # 16-B aligned (vector kernel + tail) and 4-B aligned (scalar kernel)
        buf_a = torch.full((n + 8,), 7.0, device="cuda")
        buf_p = torch.full((n + 8,), 9.0, device="cuda")
        a, q = buf_a[4 + shift:4 + shift + n], buf_p[4 + shift:4 + shift + n]
        a.copy_(avg)
        q.copy_(p)
        out = ops.swa_update(a, q, n_averaged)
        assert out.data_ptr() == a.data_ptr()
        assert torch.equal(a.cpu(), want), (n, n_averaged, shift, int((a.cpu() != want).sum()))
        assert torch.equal(q.cpu(), p)
        guard = torch.ones(n + 8, dtype=torch.bool)
        guard[4 + shift:4 + shift + n] = False
        assert (buf_a.cpu()[guard] == 7.0).all() and (buf_p.cpu()[guard] == 9.0).all()


def test_swa_update_past_the_grid_cap():
    n = 8192 * 256 * 4 + 1027
    avg, p = _pair(n, 77)
    a, q = avg.cuda(), p.cuda()
    ops.swa_update(a, q, 2)
    assert torch.equal(a.cpu(), avg + (p - avg) / torch.tensor(3))
    s = torch.zeros(n, device="cuda", dtype=torch.bfloat16)
    ops.swa_apply(a, q, s)
    assert torch.equal(q, a) and torch.equal(s, ops.cast(a, torch.bfloat16))


def test_swa_update_running_mean_of_four():
    n = 1027
    xs = [_values(n, 50 + k) for k in range(4)]
    want = xs[0].clone()
    avg = torch.zeros(n, device="cuda")
    for k, x in enumerate(xs):
        ops.swa_update(avg, x.cuda(), k)
        if k:
            want = want + (x - want) / torch.tensor(k + 1)
    assert torch.equal(avg.cpu(), want)
    mean = torch.stack(xs).double().mean(0)
    assert ((avg.cpu().double() - mean).abs() <= 1e-5 * torch.stack(xs).abs().max(0).values.double()).all()


@pytest.mark.parametrize("with_shadow", [True, False])
@pytest.mark.parametrize("n", SIZES)
def test_swa_apply_writes_master_and_shadow(n, with_shadow):
    avg = _values(n, 7 * n % 991)
    for shift in (0, 1):
        buf_p = torch.full((n + 8,), 9.0, device="cuda")
        buf_s = torch.full((n + 8,), 5.0, device="cuda", dtype=torch.bfloat16)
        a = torch.empty(n + 8, device="cuda")[4 + shift:4 + shift + n].copy_(avg)
        p, s = buf_p[4 + shift:4 + shift + n], buf_s[4 + shift:4 + shift + n]
        ops.swa_apply(a, p, s if with_shadow else None)
        assert torch.equal(p.cpu(), avg) and torch.equal(a.cpu(), avg)
        guard = torch.ones(n + 8, dtype=torch.bool)
        guard[4 + shift:4 + shift + n] = False
        assert (buf_p.cpu()[guard] == 9.0).all() and (buf_s.cpu()[guard] == 5.0).all()
        if with_shadow:
            assert torch.equal(s, ops.cast(a.contiguous(), torch.bfloat16))
            assert torch.equal(s.cpu(), avg.to(torch.bfloat16))  # round to nearest even, as torch
        else:
            assert (buf_s == 5.0).all()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_arena_swa_buffer_update_apply(dtype):
    g = torch.Generator().manual_seed(3)
    params = [("a.weight", torch.nn.Parameter(torch.randn(33, 7, generator=g))),
              ("a.bias", torch.nn.Parameter(torch.randn(33, generator=g))),
              ("frozen", torch.nn.Parameter(torch.randn(5, 5, generator=g)))]
    arena = ParamArena(params, ["a.weight", "a.bias"], dtype, torch.device("cuda"))
    assert arena.swa is None
    buf = arena.swa_buffer()
    assert buf is arena.swa_buffer() and buf.shape == arena.data.shape and buf.dtype == torch.float32
    ptrs = (arena.data.data_ptr(), arena.shadow.data_ptr() if arena.shadow is not None else None)
    arena.exp_avg.fill_(0.25)
    arena.exp_avg_sq.fill_(0.5)
    snaps = []
    for k in range(3):
        snaps.append(arena.data.cpu().clone())
        arena.swa_update(k)
        arena.data[: arena.n_grad].mul_(1.0 + 0.37 * (k + 1)).add_(0.01 * (k + 1))  # "training": frozen untouched
        arena.refresh_shadow()
    want = snaps[0].clone()
    for k in (1, 2):
        want = want + (snaps[k] - want) / torch.tensor(k + 1)
    live = arena.data.cpu().clone()
    assert torch.equal(arena.swa.cpu(), want) and not torch.equal(live, want)
    arena.swa_apply()
    assert torch.equal(arena.data.cpu(), want)
    assert (arena.data.data_ptr(), arena.shadow.data_ptr() if arena.shadow is not None else None) == ptrs
    if arena.shadow is not None:
        assert torch.equal(arena.shadow, ops.cast(arena.data, torch.bfloat16))
    for name, p in params:  # the parameters are views of the arena: they show the average
        o = arena.offsets[name]
        assert torch.equal(p.data.cpu().reshape(-1), want[o:o + p.numel()])
    o = arena.offsets["frozen"]
    assert torch.equal(want[o:o + 25], snaps[0][o:o + 25])  # a frozen parameter averages to itself
    assert (arena.exp_avg == 0.25).all() and (arena.exp_avg_sq == 0.5).all()
