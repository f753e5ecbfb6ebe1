"""Optimizer + schedule over the flat parameter arena.

ArenaAdamW = torch.optim.AdamW(trainable, lr, weight_decay, betas) as configured
by SAM2LightningModule.configure_optimizers (trainer.py:117-135: eps/amsgrad of
the YAML are NOT forwarded, so eps=1e-8, amsgrad=False) preceded by Lightning's
gradient_clip_val=1.0 (clip_grad_norm_, norm type 2).  One reduction kernel pair
computes the global norm and clip factor on the device; one fused kernel
applies clip + AdamW and refreshes the bf16 shadow weights -- no host sync.

Parameters whose gradient is None in the reference (never reached by the
step) are outside the gradient arena, so AdamW skips them exactly like torch.
"""
from __future__ import annotations

import math

import torch

from ..kernels import ops


class ArenaAdamW:
    def __init__(self, arena, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, max_grad_norm=1.0):
        self.arena = arena
        self.lr = float(lr)
        self.betas = tuple(float(b) for b in betas)
        self.eps = float(eps)
        self.weight_decay = float(weight_decay)
        self.max_grad_norm = float(max_grad_norm) if max_grad_norm else 0.0
        self.step_count = 0
        dev = arena.device
        self._partial = torch.empty(1024, device=dev)
        self.norm_out = torch.zeros(2, device=dev)  # [grad norm, clip coefficient]
        self.param_groups = [{"lr": self.lr}]

    def step(self, lr=None, grad_scale=1.0):
        """grad_scale multiplies the stored gradients (1/world after a SUM all-reduce)"""
        a = self.arena
        if a.n_grad == 0:
            return
        self.step_count += 1
        if lr is not None:
            self.param_groups[0]["lr"] = float(lr)
        lr = self.param_groups[0]["lr"]
        g = a.grad_region()
        ops.grad_norm(g, self.max_grad_norm, self._partial, self.norm_out, grad_scale)
        shadow = a.shadow[: a.n_grad] if a.shadow is not None else None
        ops.adamw(a.data[: a.n_grad], g, a.exp_avg[: a.n_grad], a.exp_avg_sq[: a.n_grad], self.norm_out, lr,
                  self.betas[0], self.betas[1], self.eps, self.weight_decay, self.step_count, shadow)

    def zero_grad(self):
        self.arena.zero_grad()

    # ---- state in torch.optim.AdamW's layout (the reference's optimizer under Lightning)
    def _torch_group(self):
        g = dict(_torch_adamw_defaults())
        g.update(lr=self.param_groups[0]["lr"], betas=self.betas, eps=self.eps, weight_decay=self.weight_decay,
                 amsgrad=False)
        return g

    def state_dict(self):
        """What `torch.optim.AdamW([p for p in model.parameters() if p.requires_grad], ...).state_dict()`
        holds for the reference's optimizer: param_groups[0] with lr / betas / eps / weight_decay / amsgrad
        False (and torch's other defaults) and params = [0..n); state[i] = {step, exp_avg, exp_avg_sq} in
        the parameter's shape for the parameters inside the gradient arena -- the others never receive a
        gradient, so torch has no state for them.  Before the first step torch has no state at all.  One
        device -> host copy per moment buffer; the entries are host views of the two copies."""
        a = self.arena
        names = a.trainable_names()
        state = {}
        if self.step_count > 0:
            avg, sq = a.split(a.exp_avg.detach().cpu(), "grad"), a.split(a.exp_avg_sq.detach().cpu(), "grad")
            for i, n in enumerate(names):
                if n in avg:
                    state[i] = {"step": torch.tensor(float(self.step_count)), "exp_avg": avg[n], "exp_avg_sq": sq[n]}
        group = self._torch_group()
        group["params"] = list(range(len(names)))
        return {"state": state, "param_groups": [group]}

    def plan_load(self, sd):
        """Everything load_state_dict checks and builds, without touching the arena: (step, lr, exp_avg,
        exp_avg_sq) with the two moments as host buffers of the gradient region's length, padding zero.
        Accepts torch's layout (state / param_groups) and this class's earlier flat dict (step, lr, exp_avg
        and exp_avg_sq of the arena's length).  What does not fit the trainable set raises ValueError naming
        the first offender."""
        a = self.arena
        length = a.exp_avg.numel()
        if "state" not in sd or "param_groups" not in sd:  # the flat dict of earlier files
            for k in ("exp_avg", "exp_avg_sq"):
                if tuple(sd[k].shape) != (length,):
                    raise ValueError(f"optimizer state: flat {k} has {tuple(sd[k].shape)} elements, the gradient "
                                     f"arena {length}")
            return (int(sd["step"]), float(sd["lr"]), sd["exp_avg"].detach().float().cpu(),
                    sd["exp_avg_sq"].detach().float().cpu())
        names = a.trainable_names()
        groups = sd["param_groups"]
        n_file = sum(len(g["params"]) for g in groups)
        if len(groups) != 1 or n_file != len(names):
            first = names[n_file] if n_file < len(names) else f"index {len(names)} of the file"
            raise ValueError(f"optimizer state: {n_file} parameters in {len(groups)} group(s) in the file, "
                             f"{len(names)} trainable parameters in one group in the model (first without a "
                             f"counterpart: {first})")
        index = {int(i): n for i, n in zip(groups[0]["params"], names)}
        in_arena = set(a.grad_names)
        state = sd["state"]
        avg, sq, steps = {}, {}, {}
        for i, st in state.items():
            n = index.get(int(i))
            if n is None:
                raise ValueError(f"optimizer state: index {i} is not in the file's param_groups")
            if n not in in_arena:
                raise ValueError(f"optimizer state: index {i} ({n}) has moments in the file, but the step never "
                                 "gives it a gradient here (it is outside the gradient arena)")
            avg[n], sq[n], steps[n] = st["exp_avg"], st["exp_avg_sq"], int(float(st["step"]))
        if not state:
            zeros = torch.zeros(length, dtype=torch.float32)
            return 0, float(groups[0]["lr"]), zeros, zeros.clone()
        flat_avg = a.join(avg, "grad", "optimizer state exp_avg")
        flat_sq = a.join(sq, "grad", "optimizer state exp_avg_sq")
        step = steps[a.grad_names[0]]
        for n in a.grad_names:
            if steps[n] != step:
                raise ValueError(f"optimizer state: parameter {n!r} is at step {steps[n]}, {a.grad_names[0]!r} at "
                                 f"{step}; the arena AdamW keeps one step count")
        return step, float(groups[0]["lr"]), flat_avg, flat_sq

    def apply_load(self, plan):
        step, lr, avg, sq = plan
        self.arena.exp_avg.copy_(avg)
        self.arena.exp_avg_sq.copy_(sq)
        self.step_count = int(step)
        self.param_groups[0]["lr"] = float(lr)

    def load_state_dict(self, sd):
        self.apply_load(self.plan_load(sd))


_TORCH_DEFAULTS = {}


def _torch_adamw_defaults():
    """the keys a param group of this torch's AdamW carries besides `params` (maximize, foreach, capturable,
    ...: they differ between torch versions, and a loaded group that misses one breaks torch's step)"""
    if not _TORCH_DEFAULTS:
        g = torch.optim.AdamW([torch.nn.Parameter(torch.zeros(1))]).param_groups[0]
        _TORCH_DEFAULTS.update({k: v for k, v in g.items() if k != "params"})
    return _TORCH_DEFAULTS


def cosine_with_warmup(base_lr, num_warmup_steps, num_training_steps, num_cycles=0.5):
    """transformers.get_cosine_schedule_with_warmup as a step -> lr function (trainer.py:137-155)"""

    def lr_at(step):
        if step < num_warmup_steps:
            return base_lr * float(step) / float(max(1, num_warmup_steps))
        progress = float(step - num_warmup_steps) / float(max(1, num_training_steps - num_warmup_steps))
        return base_lr * max(0.0, 0.5 * (1.0 + math.cos(math.pi * float(num_cycles) * 2.0 * progress)))

    return lr_at


class ArenaOptimizer(torch.optim.Optimizer):
    """The arena AdamW as a `torch.optim.Optimizer`, for Lightning's automatic optimization (the
    reference trains that way: trainer.py:117-177 returns torch AdamW, and best.yaml:105-106 puts
    gradient_clip_val: 1.0 and accumulate_grad_batches: 16 on the Trainer).

    * param_groups hold the trainable parameters; each `p.grad` is bound to the parameter's slice of
      the gradient arena (the HIP backward writes there, autograd never sets a .grad), so torch /
      Lightning code that walks `p.grad` -- GradScaler.unscale_ of precision=16, gradient-norm
      logging -- sees the real gradients;
    * zero_grad zeroes the arena and keeps the bindings (set_to_none is ignored: a None .grad would
      cut the view);
    * step(closure) runs the closure (Lightning's training_step + backward), then the fused clip +
      AdamW kernels over the whole arena with `max_grad_norm`, which
      SAM2LightningModule.configure_gradient_clipping sets from the Trainer's gradient_clip_val; with a
      process group of > 1 rank up (arena_ddp_strategy: no DistributedDataParallel wrapper) the arena
      was all-reduced before Lightning's GradScaler looked at it -- beside the staged backward by the
      graph-replayed micro-step, or by the module's backward hook (reduce_now) -- and the 1/world
      average is folded into the step's gradient scale;
    * the learning rate is param_groups[0]["lr"] (a torch LambdaLR drives it);
    * state_dict carries the arena moments in torch.optim.AdamW's layout (Lightning checkpoints)."""

    def __init__(self, arena, params, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, max_grad_norm=0.0):
        params = list(params)
        super().__init__(params, dict(lr=float(lr), betas=tuple(betas), eps=float(eps),
                                      weight_decay=float(weight_decay)))
        self.impl = ArenaAdamW(arena, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay,
                               max_grad_norm=max_grad_norm)
        self.arena = arena
        self.max_grad_norm = float(max_grad_norm or 0.0)
        self.reducer = None
        # set by SAM2LightningModule for the current accumulation window:
        self.hold_grads = False   # the next zero_grad keeps the arena (the graph-replayed micro-step filled it)
        self.window_scale = 1.0   # gradient scale of the window's arena (1/accumulate on the graph path)
        self.reduced = False      # the window's arena was already all-reduced (in the backward)
        self._bind()

    def _bind(self):
        for g in self.param_groups:
            for p in g["params"]:
                view = getattr(p, "_s2h_grad", None)
                if view is None:
                    raise ValueError("ArenaOptimizer: parameter without an arena gradient slice")
                if p.grad is None or p.grad.data_ptr() != view.data_ptr():
                    p.grad = view

    def zero_grad(self, set_to_none: bool = True):
        if self.hold_grads:  # Lightning's zero_grad after a graph-replayed first micro-batch: keep them
            self.hold_grads = False
        else:  # a new window (also after a step GradScaler skipped): fresh window state
            self.arena.zero_grad()
            self.reduced, self.window_scale = False, 1.0
        self._bind()

    @staticmethod
    def _world():
        import torch.distributed as dist
        return dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1

    def reduce_now(self):
        """SUM all-reduce of the gradient arena over the process group (DDP without the wrapper,
        arena_ddp_strategy); called from the module's backward hook on a window's last micro-batch,
        i.e. before the precision plugin's GradScaler inspects the gradients"""
        if self._world() > 1 and not self.reduced:
            if self.reducer is None:
                from .ddp import ArenaGradReducer
                self.reducer = ArenaGradReducer(self.arena.grad_region())
            self.reducer.reduce()
        self.reduced = True

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        world = self._world()
        if world > 1 and not self.reduced:  # eager path without the module's backward hook
            self.reduce_now()
        scale = self.window_scale / world
        self.reduced, self.window_scale = False, 1.0
        self.impl.max_grad_norm = self.max_grad_norm
        self.impl.step(lr=self.param_groups[0]["lr"], grad_scale=scale)
        return loss

    def state_dict(self):
        sd = self.impl.state_dict()
        sd["param_groups_lr"] = [g["lr"] for g in self.param_groups]
        return sd

    def load_state_dict(self, sd):
        self.impl.load_state_dict(sd)
        lrs = sd.get("param_groups_lr") or [self.impl.param_groups[0]["lr"]] * len(self.param_groups)
        for g, lr in zip(self.param_groups, lrs):
            g["lr"] = lr
