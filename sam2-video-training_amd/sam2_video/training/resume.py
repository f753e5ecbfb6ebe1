"""The host-side pieces of an exact resume (Trainer.fit(ckpt_path=...)): the host random
generators as checkpoint data, the train loader of an interrupted epoch positioned after the batches already
consumed, and the strict plan that turns a checkpoint's `state_dict` into one host image of the parameter arena.

Everything here plans on the host and raises ValueError before a device buffer is written; the Trainer applies
the plans with one `copy_` per arena buffer.
"""
from __future__ import annotations

import random
from typing import Any, Dict, List, Optional, Tuple

import torch

FORMAT_VERSION = 1
RESUME_KEY = "s2h_resume"


# ------------------------------------------------------------------------------------------- host randomness
def host_rng_state() -> Dict[str, Any]:
    """torch's CPU generator, Python `random` and (when numpy is importable) numpy's global generator, as
    tensors / numbers / strings only, so the checkpoint still loads with weights_only=True"""
    version, mt, gauss = random.getstate()
    out = {"torch": torch.get_rng_state().clone(),
           "python": {"version": int(version), "mt": torch.tensor(mt, dtype=torch.int64), "gauss_next": gauss},
           "numpy": None}
    try:
        import numpy as np
    except Exception:  # pragma: no cover - numpy is optional
        return out
    name, keys, pos, has_gauss, cached = np.random.get_state()
    out["numpy"] = {"name": str(name), "keys": torch.from_numpy(keys.astype("int64")), "pos": int(pos),
                    "has_gauss": int(has_gauss), "cached_gaussian": float(cached)}
    return out


def set_host_rng_state(state: Dict[str, Any]):
    torch.set_rng_state(state["torch"].to(torch.uint8).cpu())
    py = state.get("python")
    if py is not None:
        random.setstate((int(py["version"]), tuple(int(v) for v in py["mt"].tolist()), py["gauss_next"]))
    npy = state.get("numpy")
    if npy is not None:
        import numpy as np
        np.random.set_state((npy["name"], npy["keys"].numpy().astype("uint32"), int(npy["pos"]),
                             int(npy["has_gauss"]), float(npy["cached_gaussian"])))


# ------------------------------------------------------------------------------------------- data position
class _SkipIter:
    def __init__(self, it, skip):
        self.it, self.skip = it, int(skip)

    def __iter__(self):
        return self

    def prime(self):
        while self.skip > 0:
            self.skip -= 1
            if next(self.it, None) is None:
                self.skip = 0

    def __next__(self):
        self.prime()
        return next(self.it)


class SkipBatches:
    """A batch sampler that leaves out the first `skip` index batches of `batch_sampler`: the skipped clips
    are never decoded.  `prime()` performs the skip on the iterator created last.  A shuffling sampler draws
    its seed from the global generator when its first index is asked for; an uninterrupted epoch does that at
    its first batch, after the DataLoader's iterator has drawn its own base seed.  Calling prime() right
    after `iter(loader)` makes the same two draws in the same order before any batch is fetched, so the
    caller can then put the generator's later state back."""

    def __init__(self, batch_sampler, skip: int):
        self.batch_sampler = batch_sampler
        self.skip = int(skip)
        self.last = None

    def __iter__(self):
        self.last = _SkipIter(iter(self.batch_sampler), self.skip)
        return self.last

    def prime(self):
        if self.last is not None:
            self.last.prime()

    def __len__(self):
        return max(0, len(self.batch_sampler) - self.skip)


def resumed_iterator(loader, skip: int):
    """iterator over `loader`'s batches skip, skip + 1, ...  A torch DataLoader is rebuilt over the same
    dataset, workers and collate function with a SkipBatches batch sampler (skipped at the sampler level);
    any other iterable is iterated and its first `skip` batches are dropped after they were produced.
    Every draw the epoch's start makes from the global generator has been made when this returns."""
    from torch.utils.data import DataLoader
    if skip <= 0:
        return iter(loader)
    if isinstance(loader, DataLoader) and loader.batch_sampler is not None:
        kw = dict(num_workers=loader.num_workers, collate_fn=loader.collate_fn, pin_memory=loader.pin_memory,
                  timeout=loader.timeout, worker_init_fn=loader.worker_init_fn, generator=loader.generator,
                  multiprocessing_context=loader.multiprocessing_context)
        if loader.num_workers > 0:
            kw["prefetch_factor"] = loader.prefetch_factor
        sampler = SkipBatches(loader.batch_sampler, skip)
        it = iter(DataLoader(loader.dataset, batch_sampler=sampler, **kw))
        sampler.prime()
        return it
    it = iter(loader)
    for _ in range(skip):
        if next(it, None) is None:
            break
    return it


# ------------------------------------------------------------------------------------------------- weights
def plan_weights(model, state_dict: Dict[str, torch.Tensor]) -> Tuple[torch.Tensor, List[Tuple[torch.Tensor, torch.Tensor]]]:
    """(`flat`, `others`): `flat` is a host image of `model.arena.data` holding the checkpoint's parameters
    (alignment padding zero), `others` the (tensor of the model, value) pairs of the state dict's entries that
    live outside the arena (buffers).  Strict on names and shapes; nothing of the model is written."""
    arena = model.arena
    own = model.state_dict()
    for k, v in own.items():
        if k not in state_dict:
            raise ValueError(f"checkpoint state_dict: no entry for {k!r}")
        if tuple(state_dict[k].shape) != tuple(v.shape):
            raise ValueError(f"checkpoint state_dict: {k!r} has shape {tuple(state_dict[k].shape)} in the file, "
                             f"{tuple(v.shape)} in the model")
    for k in state_dict:
        if k not in own:
            raise ValueError(f"checkpoint state_dict: the file's {k!r} is not in the model")
    for n in arena.order:
        if n not in own:
            raise ValueError(f"checkpoint state_dict: the model's state_dict has no parameter {n!r}")
    flat = arena.join({n: state_dict[n] for n in arena.order}, "all", "checkpoint state_dict")
    in_arena = set(arena.order)
    others = [(v, state_dict[k]) for k, v in own.items() if k not in in_arena]
    return flat, others


def first_difference(file_names: List[str], model_names: List[str]) -> Optional[str]:
    """a sentence naming the first position at which two name lists differ, or None"""
    for i, (a, b) in enumerate(zip(file_names, model_names)):
        if a != b:
            return f"position {i} is {a!r} in the file, {b!r} in the model"
    if len(file_names) > len(model_names):
        return f"the file's {file_names[len(model_names)]!r} is not trainable in the model"
    if len(model_names) > len(file_names):
        return f"the model's {model_names[len(file_names)]!r} is not trainable in the file"
    return None
