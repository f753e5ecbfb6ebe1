"""Shared by test_attention_conditioning_host.py and test_attention_conditioning_gpu.py: attention inputs
whose scores are peaked, drift along the key axis or sit at a large common offset, a float64 reference,
a replay of the flash forward's deferred-rescale rule (csrc/flash.hip) on the reference scores, and
plain torch models of that forward and of the bf16 recomputing backward.

The score of query i and key j in nats, after scale = D ** -0.5, is a_i * c_j + shift + noise: a rank-one
term along a sign direction u (every real head dim carries it), a common offset along a second sign
direction w orthogonal to u, and 0.3-sigma Gaussian noise kept orthogonal to w (so the offset moves every
score of a row by the same amount and the softmax does not see it).  Every q / k element lies on a lattice
that bf16 holds exactly, so rounding cannot tell the shifted inputs from the unshifted ones either."""
import math

import torch

LOG2E = 1.4426950408889634
GAINS = [0.0, 1.0, 2.5, 3.9, 4.0, 6.3, -4.0, -6.3]  # a_i = GAINS[i % 8]
SPIKE = 11.0           # the spike key's c_j and the spike rows' gain: 121 nats > 149 log2 units
ZERO_ROWS = (32, 48)   # one 16-row set of a wave with gain 0 between rescaling neighbours
PROFILES = ["ramp", "saw", "spike_first", "spike_last", "spike_mid", "flat"]
SHIFTS = [0.0, 60.0, -60.0]
RESCALE_LOG2 = 8.0     # flash.hip: the reference maximum moves when a tile's maximum exceeds it by more


def query_gains(Lq, profile, Lk=None):
    """a_i [Lq] float64; the spike profiles and the ramp give every 16th row (i % 16 == 9) the gain SPIKE
    (on the ramp such a row rescales at every full tile, also where 6.3 only just reaches the trigger).
    With Lk, the spike profiles also give every 16th row (i % 16 == 1) the gain ln(Lk - 1) / SPIKE, at
    which the spike key holds about half of the row's mass: such a row has the largest dq and the spike
    key's largest dk contribution, and sets the scale the gradients are compared on (without one that scale
    is left to the noise, and the bf16 backward's error in the nearly saturated rows -- their D_i comes from
    the bf16-rounded O -- is measured against a tensor maximum that happens to be small)"""
    i = torch.arange(Lq)
    a = torch.tensor(GAINS, dtype=torch.float64)[i % 8]
    if profile.startswith("spike") and Lk is not None:
        a[i % 16 == 1] = math.log(max(Lk - 1, 2)) / SPIKE
    if profile.startswith("spike") or profile == "ramp":
        a[i % 16 == 9] = SPIKE
    a[ZERO_ROWS[0]:ZERO_ROWS[1]] = 0.0
    return a


def spike_key(Lk, profile):
    if profile == "spike_first":
        return 0
    if profile == "spike_last":
        return Lk - 1
    j = Lk // 2 + 1
    return j if j % 64 else j + 3  # the middle of the key range, not on a tile boundary


def key_profile(Lk, profile):
    """c_j [Lk] float64"""
    j = torch.arange(Lk, dtype=torch.float64)
    if profile == "ramp":
        return 6.3 * j / max(Lk - 1, 1)
    if profile == "saw":
        return 6.3 * ((torch.arange(Lk) // 64) % 2).double()
    if profile == "flat":
        return torch.zeros(Lk, dtype=torch.float64)
    c = torch.zeros(Lk, dtype=torch.float64)
    c[spike_key(Lk, profile)] = SPIKE
    return c


def directions(H, D, gen):
    """sign vectors [H, D]: su random, sw = su with every second sign flipped (su . sw = 0, D even)"""
    assert D % 2 == 0
    su = torch.randint(0, 2, (H, D), generator=gen).double() * 2 - 1
    alt = torch.ones(D, dtype=torch.float64)
    alt[1::2] = -1
    return su, su * alt


NOISE_CLAMP = 0.9


def lattice(D):
    """every q / k element is a multiple of this step and below 256 steps in magnitude, so bf16 holds it
    exactly, shifted or not: the shifted and the unshifted case are then the same inputs plus an exact
    rank-one term, and their float64 softmax is the same to rounding"""
    return 2.0 ** -5 if (SPIKE + math.sqrt(60.0)) * D ** -0.25 + NOISE_CLAMP < 8 else 2.0 ** -4


def _snap(x, step):
    return torch.round(torch.as_tensor(x, dtype=torch.float64) / step) * step


def effective_shift(D, shift):
    """the offset in nats that make_qkv(..., shift) really applies (sqrt|shift| D^-1/4 snapped to the lattice)"""
    rho = _snap(math.sqrt(abs(shift)) * D ** -0.25, lattice(D)).item()
    return math.copysign(rho * rho * math.sqrt(D), shift)


def _noise(B, L, H, D, su, gen, step):
    """0.3-sigma noise on the lattice, drawn per pair of dims so that it is exactly orthogonal to sw"""
    e = _snap((0.3 * torch.randn(B, L, H, D // 2, generator=gen, dtype=torch.float64)).clamp(-NOISE_CLAMP, NOISE_CLAMP), step)
    n = torch.empty(B, L, H, D, dtype=torch.float64)
    n[..., 0::2] = e
    n[..., 1::2] = e * su[:, 0::2] * su[:, 1::2]  # e sw[2m] + n[2m + 1] sw[2m + 1] = 0
    return n


def make_qkv(B, H, Lq, Lk, D, profile, shift=0.0, Dv=None, seed=0, dtype=torch.bfloat16):
    """q [B, Lq, H, D], k [B, Lk, H, D], v [B, Lk, H, Dv or D] on the CPU in dtype (bf16 or fp32; q and k are
    exact in either).  Per element: q = noise + snap(a_i D^-1/4) su + snap(sqrt|shift| D^-1/4) sw, k alike with
    c_j and sign(shift), so the score in nats is a_i c_j + effective_shift + noise terms"""
    gen = torch.Generator().manual_seed(seed)
    step = lattice(D)
    su, sw = directions(H, D, gen)
    nq = _noise(B, Lq, H, D, su, gen, step)
    nk = _noise(B, Lk, H, D, su, gen, step)
    v = torch.randn(B, Lk, H, Dv or D, generator=gen, dtype=torch.float64)
    g = D ** -0.25
    a = _snap(query_gains(Lq, profile, Lk) * g, step).view(1, Lq, 1, 1)
    c = _snap(key_profile(Lk, profile) * g, step).view(1, Lk, 1, 1)
    rho = _snap(math.sqrt(abs(shift)) * g, step)
    q = nq + a * su + rho * sw
    k = nk + c * su + math.copysign(1.0, shift) * rho * sw
    for t in (q, k):
        assert torch.equal(t.bfloat16().double(), t), "off the bf16 lattice"
    return q.to(dtype), k.to(dtype), v.to(dtype)


def reference(q, k, v, scale, do=None, keep=None, p_drop=0.0):
    """float64 attention on the given (rounded) inputs, [B, L, H, D] layout -> dict with o [B, Lq, H, Dv],
    lse [B, H, Lq] (nats), s [B, H, Lq, Lk] (nats) and, with do, dq / dk / dv from autograd.
    keep [B, H, Lq, Lk] (bool) with p_drop: o = (P * keep / (1 - p_drop)) V and rowsum = its row sums"""
    qd, kd, vd = (t.detach().double().cpu().transpose(1, 2).clone().requires_grad_(do is not None) for t in (q, k, v))
    s = (qd @ kd.transpose(-1, -2)) * scale
    lse = torch.logsumexp(s, -1)
    p = torch.exp(s - lse[..., None])
    out = {}
    if keep is not None:
        p = p * keep.double() / (1.0 - p_drop)
        out["rowsum"] = p.sum(-1).detach()
    o = (p @ vd).transpose(1, 2)
    if do is not None:
        o.backward(do.detach().double().cpu())
        out.update(dq=qd.grad.transpose(1, 2), dk=kd.grad.transpose(1, 2), dv=vd.grad.transpose(1, 2))
    out.update(o=o.detach(), lse=lse.detach(), s=s.detach())
    return out


def regime(scores_log2, tile=64, detail=False):
    """The deferred-rescale rule on scores [..., Lq, Lk] in log2 units: per row the number of rescales
    after tile 0 and the largest tile max - reference max at which none fired (-inf when every tile did);
    detail adds the smallest tile max - reference max at which one fired (+inf when none did)"""
    Lk = scores_log2.shape[-1]
    m = scores_log2[..., :tile].amax(-1)
    count = torch.zeros_like(m, dtype=torch.int64)
    held = torch.full_like(m, -math.inf)
    fired = torch.full_like(m, math.inf)
    for k0 in range(tile, Lk, tile):
        mx = scores_log2[..., k0:k0 + tile].amax(-1)
        fire = mx > m + RESCALE_LOG2
        count += fire
        held = torch.where(fire, held, torch.maximum(held, mx - m))
        fired = torch.where(fire, torch.minimum(fired, mx - m), fired)
        m = torch.where(fire, mx, m)
    return (count, held, fired) if detail else (count, held)


def emulate_flash(q, k, v, scale, skip_rescale=False, tile=64):
    """flash_fwd_kernel's arithmetic in plain torch on one key split: 64-key tiles, fp32 scores from the
    bf16 operands, fp32 m / l / o, the reference maximum moved only past RESCALE_LOG2, P rounded to bf16
    before P V.  skip_rescale drops the o *= alpha step (the fault the structured inputs must expose).
    -> o [B, Lq, H, Dv] fp32, lse [B, H, Lq] fp32"""
    qf, kf, vf = (t.float().transpose(1, 2) for t in (q, k, v))
    B, H, Lq, _ = qf.shape
    Lk = kf.shape[2]
    sl2 = torch.tensor(scale * LOG2E, dtype=torch.float32)
    m = torch.full((B, H, Lq), -math.inf)
    l = torch.zeros(B, H, Lq)
    o = torch.zeros(B, H, Lq, vf.shape[-1])
    for k0 in range(0, Lk, tile):
        s = (qf @ kf[:, :, k0:k0 + tile].transpose(-1, -2)) * sl2
        mx = s.amax(-1)
        mn = torch.where(mx > m + RESCALE_LOG2, mx, m)
        alpha = torch.where(torch.isinf(m), torch.zeros_like(m), torch.exp2(m - mn))
        m = mn
        p = torch.exp2(s - m[..., None])
        l = l * alpha + p.sum(-1)
        if not skip_rescale:
            o = o * alpha[..., None]
        o = o + p.bfloat16().float() @ vf[:, :, k0:k0 + tile]
    return (o / l[..., None]).transpose(1, 2), (m + torch.log2(l)) / LOG2E


def structured_rows(gains, H, D, seed, stream=0):
    """[len(gains), H, D] float64 rows of make_qkv's kind for callers that lay out their own tensors: lattice
    noise + snap(gain D^-1/4) su, so row_a . row_b * D^-1/2 = gain_a gain_b + noise terms.  seed fixes su,
    stream the noise (queries and keys of one case: the same seed, different streams)"""
    gen = torch.Generator().manual_seed(seed)
    su, _ = directions(H, D, gen)
    gains = torch.as_tensor(gains, dtype=torch.float64)
    n = _noise(1, gains.numel(), H, D, su, torch.Generator().manual_seed(1000003 * (stream + 1) + seed), lattice(D))[0]
    return n + _snap(gains * D ** -0.25, lattice(D)).view(-1, 1, 1) * su


def emulate_flash_bwd(q, k, v, do, scale, o_fp32=False):
    """the bf16 flash backward's arithmetic in plain torch (flash_bwd.hip; the standard recomputation):
    O and the LSE of emulate_flash, O rounded to bf16 as the forward stores it, D_i = rowsum(dO o O) and
    P = exp2(s sl2 - lse log2e) in fp32, P and dS rounded to bf16 for their products, fp32 sums, bf16
    results.  o_fp32 keeps O unrounded (shows how much of the error is D_i's).  -> dq, dk, dv"""
    o, lse = emulate_flash(q, k, v, scale)
    o = o.transpose(1, 2)
    if not o_fp32:
        o = o.bfloat16().float()
    qf, kf, vf, dof = (t.float().transpose(1, 2) for t in (q, k, v, do))
    s = (qf @ kf.transpose(-1, -2)) * torch.tensor(scale * LOG2E, dtype=torch.float32)
    p = torch.exp2(s - (lse * LOG2E)[..., None])
    di = (dof * o).sum(-1)
    ds = (p * (dof @ vf.transpose(-1, -2) - di[..., None])).bfloat16().float()
    dv = p.bfloat16().float().transpose(-1, -2) @ dof
    dk = (ds.transpose(-1, -2) @ qf) * scale
    dq = (ds @ kf) * scale
    return tuple(t.bfloat16().transpose(1, 2) for t in (dq, dk, dv))


def row_err(o, ref, floor=1e-30):
    """max |o - ref| of each query row relative to that row's max |ref| (at least floor): [B, Lq, H]"""
    o, ref = o.detach().double().cpu(), ref.double()
    return (o - ref).abs().amax(-1) / ref.abs().amax(-1).clamp_min(floor)


def tensor_err(g, ref):
    """max |g - ref| relative to max |ref|"""
    g, ref = g.detach().double().cpu(), ref.double()
    return ((g - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()
