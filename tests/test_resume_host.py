"""Resuming a fit from a checkpoint, the parts that need no GPU: callback state at every cut point of a scripted
metric sequence, the optimizer state in torch.optim.AdamW's layout in both directions over a CPU ParamArena, the
position of the train loader inside an interrupted epoch, and the checkpoint file with its resume block.  Every
comparison is exact."""
import os
import random
import warnings
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from sam2_video.kernels.arena import ALIGN, ParamArena
from sam2_video.training import callbacks as C
from sam2_video.training import resume as R
from sam2_video.training.optim import ArenaAdamW
from test_callbacks_host import SEQ, FakeModule, FakeTrainer, _files

MON = "val/total_loss"


# ------------------------------------------------------------------------------------------------ callbacks
def _callbacks(root):
    return [C.ModelCheckpoint(monitor=MON, mode="min", save_top_k=2, save_last=True, dirpath=str(root / "ck"),
                              filename="e{epoch}", auto_insert_metric_name=False),
            C.EarlyStopping(monitor=MON, patience=3, mode="min"),
            C.StochasticWeightAveraging(swa_lrs=0.005, swa_epoch_start=3, annealing_epochs=3)]


def _base_lr(epoch):
    return 1e-3 * (1.0 - 0.1 * epoch)


def _through_a_file(obj, path):
    torch.save(obj, path)
    return torch.load(path, map_location="cpu", weights_only=True)


def _run(root, cut=None):
    """the scripted run: per epoch on_train_epoch_start, one validation, on_train_epoch_end.  `cut`: after that
    many validations the callbacks' state goes through a file into fresh callbacks built with the same
    arguments (and the trainer's own epoch rate into a fresh trainer), which finish the run."""
    os.makedirs(root, exist_ok=True)
    n = len(SEQ)
    tr, mod, cbs = FakeTrainer(root, max_epochs=n, base_lr=_base_lr), FakeModule(), _callbacks(root)
    for cb in cbs:
        cb.on_fit_start(tr, mod)
    saved, calls, lrs, stops = [], [], {}, []

    def swap():
        nonlocal tr, mod, cbs
        state = _through_a_file({"callbacks": {cb.state_key: cb.state_dict() for cb in cbs},
                                 "epoch_lr": tr.epoch_lr, "metrics": dict(tr.callback_metrics),
                                 "epoch": tr.current_epoch, "step": tr.global_step}, str(root / "state.pt"))
        saved.extend(tr.saved)
        calls.extend(mod.model.arena.calls)
        tr, mod, cbs = FakeTrainer(root, max_epochs=n, base_lr=_base_lr), FakeModule(), _callbacks(root)
        tr.epoch_lr, tr.current_epoch, tr.global_step = state["epoch_lr"], state["epoch"], state["step"]
        tr.callback_metrics.update(state["metrics"])
        for cb in cbs:
            cb.on_fit_start(tr, mod)
            cb.load_state_dict(state["callbacks"][cb.state_key])

    if cut == 0:
        swap()
    for e in range(n):
        tr.current_epoch = e
        for cb in cbs:
            cb.on_train_epoch_start(tr, mod)
        lrs[e] = tr.current_lr()
        tr.should_stop = False
        tr.validate(cbs, e, val__total_loss=SEQ[e])
        if tr.should_stop:
            stops.append(e)
        if cut == e + 1:
            swap()
        for cb in cbs:
            cb.on_train_epoch_end(tr, mod)
    for cb in cbs:
        cb.on_train_end(tr, mod)
    ck, es, swa = cbs
    saved.extend(tr.saved)
    calls.extend(mod.model.arena.calls)
    return {"files": {f: open(root / "ck" / f).read() for f in _files(root / "ck")}, "saved": saved,
            "best": (ck.best_model_path, ck.best_model_score), "kth": (ck.kth_best_model_path, ck.kth_value),
            "best_k": dict(ck.best_k_models), "last": ck.last_model_path, "current": ck.current_score,
            "stops": stops, "es": (es.wait_count, es.best_score, es.stopped_epoch, es.patience),
            "swa": (swa.n_averaged, swa.swa_start, swa.swa_end, swa._latest_update_epoch, swa.applied),
            "swa_calls": [c for c in calls if c != "buffer"], "lrs": lrs, "final_lr": tr.epoch_lr}


@pytest.fixture(scope="module")
def straight(tmp_path_factory):
    return _run(tmp_path_factory.mktemp("straight") / "run")


def test_the_scripted_run_exercises_every_callback(straight):
    assert straight["stops"] == [4]  # patience 3: 0.4, 0.3 (a tie), 0.6; then 0.1 improves
    assert sorted(straight["files"]) == ["e3.ckpt", "e5.ckpt", "last.ckpt"]
    assert straight["swa"] == (4, 2, 5, 5, True)  # (n_averaged, swa_start, swa_end, latest update, applied)
    assert straight["lrs"][0] == _base_lr(0) and straight["lrs"][2] == _base_lr(2) and straight["lrs"][3] != _base_lr(3)


@pytest.mark.parametrize("cut", range(len(SEQ) + 1))
def test_callbacks_resume_at_every_cut_point(tmp_path, straight, cut):
    got = _run(tmp_path / "run", cut)
    want = straight
    base = os.path.basename  # (the two runs live in different directories)
    assert got["files"] == want["files"]
    assert [base(p) for p in got["saved"]] == [base(p) for p in want["saved"]]
    assert (base(got["best"][0]), got["best"][1]) == (base(want["best"][0]), want["best"][1])
    assert (base(got["kth"][0]), got["kth"][1]) == (base(want["kth"][0]), want["kth"][1])
    assert {base(p): v for p, v in got["best_k"].items()} == {base(p): v for p, v in want["best_k"].items()}
    assert base(got["last"]) == base(want["last"]) and got["current"] == want["current"]
    assert got["es"] == want["es"]
    assert got["stops"] == want["stops"]
    assert got["swa"] == want["swa"] and got["swa_calls"] == want["swa_calls"]
    assert got["lrs"] == want["lrs"] and got["final_lr"] == want["final_lr"]


def test_state_keys_tell_callbacks_apart_and_inert_ones_have_no_state(tmp_path):
    a, b = C.ModelCheckpoint(monitor=MON), C.ModelCheckpoint(monitor="val/iou", mode="max")
    assert a.state_key != b.state_key and a.state_key.startswith("ModelCheckpoint")
    assert C.EarlyStopping(monitor=MON).state_key.startswith("EarlyStopping")
    assert C.StochasticWeightAveraging(swa_lrs=0.1).state_key == "StochasticWeightAveraging"
    assert C.LearningRateMonitor().state_dict() == {} and C.Callback().state_key == "Callback"
    C.ModelSummary().load_state_dict({})


def test_model_checkpoint_in_another_directory_keeps_only_the_best_path(tmp_path):
    a = C.ModelCheckpoint(monitor=MON, dirpath=str(tmp_path / "a"), save_top_k=2)
    tr = FakeTrainer(tmp_path)
    for e, v in enumerate([0.5, 0.3]):
        tr.validate([a], e, val__total_loss=v)
    b = C.ModelCheckpoint(monitor=MON, dirpath=str(tmp_path / "b"), save_top_k=2)
    with pytest.warns(UserWarning, match="dirpath"):
        b.load_state_dict(a.state_dict())
    assert b.best_model_path == a.best_model_path and b.best_k_models == {} and b.best_model_score is None


# ---------------------------------------------------------------------------------------- optimizer layout
class Toy(torch.nn.Module):
    """a frozen parameter first (torch's index order differs from the arena's), a packed trainable group, a
    trainable parameter the step never reaches (outside the gradient arena), a size that is no multiple of 64"""

    def __init__(self, seed=0):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.frozen = torch.nn.Parameter(torch.randn(5, 5, generator=g), requires_grad=False)
        self.odd = torch.nn.Parameter(torch.randn(33, 3, generator=g))
        self.outside = torch.nn.Parameter(torch.randn(7, generator=g))
        self.q = torch.nn.Linear(8, 8)
        self.k = torch.nn.Linear(8, 8)
        self.register_buffer("table", torch.randn(3, generator=g))
        with torch.no_grad():
            for p in (self.q.weight, self.q.bias, self.k.weight, self.k.bias):
                p.copy_(torch.randn(p.shape, generator=g))
        self.arena = None

    strip_lightning_prefix = staticmethod(lambda ck: {k[len("model."):]: v for k, v in ck["state_dict"].items()})

    def load(self):
        named = list(self.named_parameters())
        grad_names = [n for n, p in named if p.requires_grad and n != "outside"]
        self.arena = ParamArena(named, grad_names, torch.float32, torch.device("cpu"),
                                groups=[["q.weight", "k.weight"]])
        return self


def _toy(seed=0):
    toy = Toy(seed).load()
    opt = ArenaAdamW(toy.arena, lr=3e-4, betas=(0.8, 0.95), weight_decay=0.02, max_grad_norm=1.0)
    return toy, opt


def _reference_params(toy):
    return [p for p in toy.parameters() if p.requires_grad]  # reference training/trainer.py:120-130


def _padding_mask(arena):
    mask = torch.ones(arena.exp_avg.numel(), dtype=torch.bool)
    for n in arena.grad_names:
        mask[arena.offsets[n]:arena.offsets[n] + arena.params[n].numel()] = False
    return mask


def test_toy_arena_has_the_members_the_layout_test_needs():
    toy, _ = _toy()
    a = toy.arena
    assert a.group_is_packed(["q.weight", "k.weight"]) and a.offsets["k.weight"] == a.offsets["q.weight"] + 64
    assert "outside" not in a.grad_names and "frozen" not in a.grad_names and toy.outside.requires_grad
    assert a.params["odd"].numel() % ALIGN and _padding_mask(a).any()
    assert a.trainable_names() == ["odd", "outside", "q.weight", "q.bias", "k.weight", "k.bias"]


def test_state_dict_is_what_torch_adamw_holds_and_loads_into_one():
    toy, opt = _toy()
    a = toy.arena
    assert opt.state_dict()["state"] == {}  # torch has no state before the first step
    n = a.exp_avg.numel()
    a.exp_avg.copy_(torch.arange(n, dtype=torch.float32) + 0.5)
    a.exp_avg_sq.copy_(torch.arange(n, dtype=torch.float32) * 2 + 1000)
    opt.step_count = 5
    sd = opt.state_dict()
    params = _reference_params(toy)
    names = a.trainable_names()
    group = sd["param_groups"][0]
    assert len(sd["param_groups"]) == 1 and group["params"] == list(range(len(params)))
    assert (group["lr"], group["betas"], group["eps"], group["weight_decay"], group["amsgrad"]) == \
        (3e-4, (0.8, 0.95), 1e-8, 0.02, False)
    assert sorted(sd["state"]) == [i for i, name in enumerate(names) if name in a.grad_names]
    assert names.index("outside") not in sd["state"]
    ref = torch.optim.AdamW(params, lr=1.0)
    ref.load_state_dict(sd)
    for i, (name, p) in enumerate(zip(names, params)):
        if name == "outside":
            assert p not in ref.state
            continue
        o = a.offsets[name]
        for key, flat in (("exp_avg", a.exp_avg), ("exp_avg_sq", a.exp_avg_sq)):
            assert sd["state"][i][key].shape == p.shape
            assert torch.equal(sd["state"][i][key].reshape(-1), flat[o:o + p.numel()])
            assert torch.equal(ref.state[p][key], sd["state"][i][key])
        assert float(sd["state"][i]["step"]) == 5.0 == float(ref.state[p]["step"])
    assert ref.param_groups[0]["lr"] == 3e-4 and ref.param_groups[0]["betas"] == (0.8, 0.95)
    for p in params[:1] + params[2:]:
        p.grad = torch.ones_like(p)
    ref.step()  # the loaded group is complete: torch's own step runs on it
    assert float(ref.state[params[0]]["step"]) == 6.0
    # the file form: one storage per moment buffer, still torch-loadable
    assert sd["state"][0]["exp_avg"].untyped_storage().data_ptr() == sd["state"][2]["exp_avg"].untyped_storage().data_ptr()


def _stepped_torch_adamw(toy, steps=2):
    params = _reference_params(toy)
    ref = torch.optim.AdamW(params, lr=2e-4, betas=(0.8, 0.95), weight_decay=0.02)
    g = torch.Generator().manual_seed(7)
    for _ in range(steps):
        for name, p in zip(toy.arena.trainable_names(), params):
            p.grad = None if name == "outside" else torch.randn(p.shape, generator=g)
        ref.step()
    return ref, params


def test_a_real_torch_adamw_state_loads_into_the_arena():
    toy, opt = _toy()
    a = toy.arena
    a.exp_avg.fill_(9.0)  # (padding included: the load must zero it)
    a.exp_avg_sq.fill_(9.0)
    ref, params = _stepped_torch_adamw(toy)
    opt.load_state_dict(ref.state_dict())
    assert opt.step_count == 2 and opt.param_groups[0]["lr"] == 2e-4
    for name, p in zip(a.trainable_names(), params):
        if name == "outside":
            continue
        o = a.offsets[name]
        assert torch.equal(a.exp_avg[o:o + p.numel()], ref.state[p]["exp_avg"].reshape(-1))
        assert torch.equal(a.exp_avg_sq[o:o + p.numel()], ref.state[p]["exp_avg_sq"].reshape(-1))
    pad = _padding_mask(a)
    assert not a.exp_avg[pad].any() and not a.exp_avg_sq[pad].any()
    # and back out again, bit for bit
    back = opt.state_dict()
    for i, p in enumerate(params):
        if p in ref.state:
            assert torch.equal(back["state"][i]["exp_avg_sq"], ref.state[p]["exp_avg_sq"])


def test_the_flat_dict_of_earlier_files_still_loads():
    toy, opt = _toy()
    n = toy.arena.exp_avg.numel()
    flat = {"step": 7, "lr": 1e-5, "exp_avg": torch.randn(n), "exp_avg_sq": torch.rand(n)}
    opt.load_state_dict(flat)
    assert opt.step_count == 7 and opt.param_groups[0]["lr"] == 1e-5
    assert torch.equal(toy.arena.exp_avg, flat["exp_avg"]) and torch.equal(toy.arena.exp_avg_sq, flat["exp_avg_sq"])
    with pytest.raises(ValueError, match="flat exp_avg"):
        opt.load_state_dict(dict(flat, exp_avg=torch.zeros(n + 64)))


def test_a_state_that_does_not_fit_raises_and_leaves_the_moments_alone():
    toy, opt = _toy()
    a = toy.arena
    a.exp_avg.copy_(torch.arange(a.exp_avg.numel(), dtype=torch.float32))
    before = a.exp_avg.clone()
    ref, params = _stepped_torch_adamw(toy)
    names = a.trainable_names()

    def broken(edit):
        sd = ref.state_dict()
        sd["state"] = {i: dict(st) for i, st in sd["state"].items()}
        edit(sd)
        return sd

    i_odd, i_out = names.index("odd"), names.index("outside")
    cases = [
        (lambda sd: sd["state"][i_odd].update(exp_avg=torch.zeros(3, 33)), "'odd' has shape"),
        (lambda sd: sd["state"].update({i_out: dict(sd["state"][i_odd])}), "outside"),
        (lambda sd: sd["state"].pop(names.index("q.bias")), "'q.bias'"),
        (lambda sd: sd["param_groups"][0].update(params=list(range(len(names) - 1))), "k.bias"),
        (lambda sd: sd["state"][names.index("k.weight")].update(step=torch.tensor(3.0)), "'k.weight' is at step 3"),
    ]
    for edit, match in cases:
        with pytest.raises(ValueError, match=match):
            opt.load_state_dict(broken(edit))
        assert torch.equal(a.exp_avg, before) and opt.step_count == 0


# ------------------------------------------------------------------------------------------- data position
class Counting:
    """a dataset wrapper that counts what is decoded"""

    def __init__(self, ds):
        self.ds, self.fetched = ds, []

    def __len__(self):
        return len(self.ds)

    def __getitem__(self, i):
        self.fetched.append(i)
        return self.ds[i]


def _data_module(n_clips):
    from sam2_video.training.trainer import SAM2LightningDataModule
    dm = SAM2LightningDataModule({"image_size": 16, "video_clip_length": 1, "num_categories": 2, "batch_size": 1,
                                  "num_workers": 0, "synthetic_clips": n_clips, "synthetic_objects": 2},
                                 train_shuffle=True)
    dm.setup("fit")
    dm.train_dataset = Counting(dm.train_dataset)
    return dm


def _host_prompt_stage():
    """what a training step draws between two batches (utils/prompts.py: clicks from the global generator)"""
    return torch.randperm(11), random.random(), np.random.rand()


def _epoch(loader, resume=None):
    """one epoch's batches with a prompt stage after each; returns (images, draws, states before and after each
    batch).  `resume` = (epoch-start torch state, batches done, host state at that moment)."""
    if resume is None:
        start = torch.get_rng_state()
        it, first = iter(loader), 0
    else:
        start, first, now = resume
        torch.set_rng_state(start)
        it = R.resumed_iterator(loader, first)
        R.set_host_rng_state(now)
    images, draws, states = [], [], [R.host_rng_state()]
    for batch in it:
        images.append(batch.img_batch.clone())
        draws.append(_host_prompt_stage())
        states.append(R.host_rng_state())
    return start, images, draws, states


def _same_draws(a, b):
    return len(a) == len(b) and all(torch.equal(x[0], y[0]) and x[1:] == y[1:] for x, y in zip(a, b))


def _check_tail(loader, ds, n):
    torch.manual_seed(5)
    random.seed(5)
    np.random.seed(5)
    start, images, draws, states = _epoch(loader)
    assert len(images) == n
    final = torch.get_rng_state()
    order = list(ds.fetched)
    for k in range(1, n + 1):
        torch.manual_seed(1000 + k)  # whatever a fresh process holds
        random.seed(1000 + k)
        np.random.seed(1000 + k)
        del ds.fetched[:]
        _, tail, tail_draws, _ = _epoch(loader, (start, k, states[k]))
        assert len(tail) == n - k and all(torch.equal(a, b) for a, b in zip(tail, images[k:]))
        assert _same_draws(tail_draws, draws[k:])
        assert ds.fetched == order[k:]  # skipped in the sampler: the consumed clips are not decoded again
        assert torch.equal(torch.get_rng_state(), final)
    return order


def test_resumed_loader_yields_the_tail_of_the_shuffled_epoch():
    n = 7
    dm = _data_module(n)
    loader = dm.train_dataloader()
    order = _check_tail(loader, dm.train_dataset, n)
    assert sorted(order) == list(range(n)) and order != list(range(n))  # (shuffled)
    # another epoch-start state gives another order: the order does come from the saved state
    torch.manual_seed(6)
    del dm.train_dataset.fetched[:]
    _epoch(loader)
    assert dm.train_dataset.fetched != order


@pytest.mark.parametrize("rank", [0, 1])
def test_resumed_loader_under_a_distributed_sampler(rank):
    from torch.utils.data import DataLoader, DistributedSampler

    from sam2_video.data.synthetic import sam2_collate_fn
    dm = _data_module(7)
    ds = dm.train_dataset
    sampler = DistributedSampler(ds, num_replicas=2, rank=rank, shuffle=True)  # (no process group needed)
    loader = DataLoader(ds, batch_size=1, sampler=sampler, collate_fn=sam2_collate_fn)
    sampler.set_epoch(3)
    order = _check_tail(loader, ds, 4)
    g = torch.Generator().manual_seed(3)
    want = torch.randperm(7, generator=g).tolist()
    want = (want + want[:1])[rank::2]
    assert order == want


def test_an_iterable_that_is_no_dataloader_drops_the_batches_it_produced():
    assert list(R.resumed_iterator([10, 11, 12, 13], 3)) == [13]
    assert list(R.resumed_iterator([10, 11], 5)) == [] and list(R.resumed_iterator([10, 11], 0)) == [10, 11]


# ---------------------------------------------------------------------------------------------------- file
def _fitting_trainer(tmp_path, toy, opt, micro_step=5, accumulate=3):
    """a Trainer in the state fit() keeps while it runs, over the CPU toy (the step itself needs the GPU)"""
    from sam2_video.training.trainer import Trainer
    cbs = [C.EarlyStopping(monitor=MON, patience=3), C.LearningRateMonitor(),
           C.ModelCheckpoint(monitor=MON, dirpath=str(tmp_path / "ck"), save_top_k=-1, save_last=True)]
    tr = Trainer(max_epochs=3, accumulate_grad_batches=accumulate, callbacks=cbs)
    module = SimpleNamespace(model=toy, optimizer=opt, lr_at=lambda step: 1e-4 * (1 + step))
    tr.module = module
    tr.runner = SimpleNamespace(micro_step=micro_step, accumulate=accumulate, global_step=micro_step // accumulate,
                                seed_base=1234, lr_override=0.0125)
    tr.global_step, tr.current_epoch = tr.runner.global_step, 1
    tr._batches_done, tr._epoch_finished, tr._rng_epoch_start = 2, False, torch.get_rng_state()
    tr.callback_metrics.update({MON: 0.25, "train/total_loss": 1.5})
    tr.history.append({"train/total_loss": 1.5, "step": 1, "epoch": 0, "time_s": 0.1})
    tr.val_history.append({MON: 0.25, "step": 1})
    return tr, module


def _saved(tmp_path, seed=0, **kw):
    toy, opt = _toy(seed)
    a = toy.arena
    n = a.exp_avg.numel()
    a.exp_avg.copy_(torch.arange(n, dtype=torch.float32) * ~_padding_mask(a))
    a.exp_avg_sq.copy_(torch.arange(n, dtype=torch.float32) * 3 * ~_padding_mask(a))
    a.grad.copy_(torch.arange(n, dtype=torch.float32) * -1 * ~_padding_mask(a))
    a.swa_buffer().copy_(a.join({name: torch.full(a.params[name].shape, i + 0.25)
                                 for i, name in enumerate(a.order)}, "all"))
    opt.step_count = 1
    tr, module = _fitting_trainer(tmp_path, toy, opt, **kw)
    tr.callbacks[0].wait_count, tr.callbacks[0].best_score = 2, 0.125
    path = str(tmp_path / "mid.ckpt")
    torch.manual_seed(21)
    random.seed(21)
    np.random.seed(21)
    _host_prompt_stage()
    tr.save_checkpoint(path)
    after = _host_prompt_stage()
    return tr, module, path, after


def test_the_file_loads_with_weights_only_and_carries_the_resume_block(tmp_path):
    tr, module, path, after = _saved(tmp_path)
    a = module.model.arena
    assert not os.path.exists(path + ".part")
    ck = torch.load(path, map_location="cpu", weights_only=True)
    assert set(ck) == {"state_dict", "optimizer_states", "global_step", "epoch", "lr_schedulers", "callbacks",
                       R.RESUME_KEY}
    assert all(k.startswith("model.") for k in ck["state_dict"]) and "model.table" in ck["state_dict"]
    assert (ck["global_step"], ck["epoch"]) == (1, 1)
    assert ck["lr_schedulers"][0]["last_epoch"] == 1 and ck["lr_schedulers"][0]["base_lrs"] == [3e-4]
    es, lrm, mc = tr.callbacks
    assert set(ck["callbacks"]) == {es.state_key, mc.state_key}  # (the inert callback has no state)
    assert ck["callbacks"][es.state_key] == {"wait_count": 2, "stopped_epoch": 0, "best_score": 0.125, "patience": 3}
    assert ck["callbacks"][mc.state_key]["kth_value"] == float("inf")
    b = ck[R.RESUME_KEY]
    assert (b["version"], b["world_size"], b["accumulate"], b["micro_step"], b["batches_done"], b["epoch_finished"],
            b["seed_base"], b["lr_override"]) == (1, 1, 3, 5, 2, False, 1234, 0.0125)
    assert b["callback_metrics"] == tr.callback_metrics and b["history"] == tr.history
    assert b["val_history"] == tr.val_history and b["trainable"] == a.trainable_names()
    # arena-shaped tensors: per parameter name, in the parameter's shape
    grads = b["ranks"][0]["grads"]
    assert sorted(grads) == sorted(a.grad_names) and sorted(b["swa"]) == sorted(a.order)
    for name in a.grad_names:
        o, p = a.offsets[name], a.params[name]
        assert grads[name].shape == p.shape and torch.equal(grads[name].reshape(-1), a.grad[o:o + p.numel()])
    for name in a.order:
        o, p = a.offsets[name], a.params[name]
        assert torch.equal(b["swa"][name].reshape(-1), a.swa[o:o + p.numel()])
    # the host generators survive the file
    assert torch.equal(b["ranks"][0]["epoch_start"], tr._rng_epoch_start)
    _host_prompt_stage()
    R.set_host_rng_state(b["ranks"][0]["now"])
    again = _host_prompt_stage()
    assert torch.equal(again[0], after[0]) and again[1:] == after[1:]
    # torch's own AdamW reads the optimizer entry
    torch.optim.AdamW(_reference_params(module.model)).load_state_dict(ck["optimizer_states"][0])


def test_a_closed_window_stores_no_gradients(tmp_path):
    tr, module, path, _ = _saved(tmp_path, micro_step=6)
    assert torch.load(path, weights_only=True)[R.RESUME_KEY]["ranks"][0]["grads"] is None


def _fresh(tmp_path, seed=3, **kw):
    toy, opt = _toy(seed)
    tr, module = _fitting_trainer(tmp_path, toy, opt, **kw)
    tr.runner.micro_step = tr.runner.global_step = 0
    tr.history.clear(), tr.val_history.clear(), tr.callback_metrics.clear()
    return tr, module


def test_plan_and_apply_put_every_piece_back(tmp_path):
    src_tr, src, path, _ = _saved(tmp_path)
    tr, module = _fresh(tmp_path)
    a, sa = module.model.arena, src.model.arena
    a.swa_buffer()
    assert not torch.equal(a.data, sa.data)
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # this build's own file: nothing to warn about
        plan = tr._plan_resume(path, module, tr.runner, 0, 1)
    assert (plan["mid_epoch"], plan["skip"], plan["start_epoch"], plan["complete"]) == (True, 2, 1, False)
    tr._apply_resume(plan, module, tr.runner)
    for cb in tr.callbacks:
        cb.on_fit_start(tr, module)
    tr._restore_callbacks(plan, module)
    tr._restore_books(plan)
    for name in ("data", "grad", "exp_avg", "exp_avg_sq", "swa"):
        assert torch.equal(getattr(a, name), getattr(sa, name)), name
    assert torch.equal(module.model.table, src.model.table)
    assert all(torch.equal(p, q) for p, q in zip(module.model.parameters(), src.model.parameters()))
    assert module.model.odd.data_ptr() == a.data[a.offsets["odd"]:].data_ptr()  # still views of the arena
    run = tr.runner
    assert (run.micro_step, run.global_step, run.seed_base, run.lr_override) == (5, 1, 1234, 0.0125)
    assert (tr.global_step, tr.current_epoch, tr._batches_done, tr._epoch_finished) == (1, 1, 2, False)
    assert module.optimizer.step_count == 1 and module.optimizer.param_groups[0]["lr"] == 3e-4
    assert tr.callbacks[0].wait_count == 2 and tr.callbacks[0].best_score == 0.125
    assert tr.history == src_tr.history and tr.val_history == src_tr.val_history
    assert tr.callback_metrics == src_tr.callback_metrics
    # a run that is over: epoch 1 finished of max_epochs 2
    ck = torch.load(path, weights_only=True)
    ck[R.RESUME_KEY]["epoch_finished"] = True
    torch.save(ck, path)
    tr.max_epochs = 2
    assert tr._plan_resume(path, module, tr.runner, 0, 1)["complete"]
    tr.max_epochs = 3  # ... and a larger max_epochs goes on with epoch 2
    plan = tr._plan_resume(path, module, tr.runner, 0, 1)
    assert (plan["complete"], plan["mid_epoch"], plan["start_epoch"], plan["skip"]) == (False, False, 2, 0)


def test_a_file_without_the_resume_block_takes_the_foreign_path_and_warns(tmp_path):
    _, src, path, _ = _saved(tmp_path)
    ck = torch.load(path, weights_only=True)
    want = src.model.arena.data.clone()
    ref, _ = _stepped_torch_adamw(src.model)  # (steps the source's parameters: `want` is what the file holds)
    foreign = {"state_dict": ck["state_dict"], "optimizer_states": [ref.state_dict()], "global_step": 4, "epoch": 2,
               "lr_schedulers": [], "callbacks": {}}
    torch.save(foreign, path)
    tr, module = _fresh(tmp_path)
    with pytest.warns(UserWarning, match="position inside epoch 2 is not known") as rec:
        plan = tr._plan_resume(path, module, tr.runner, 0, 1)
    assert len(rec) == 1
    assert (plan["mid_epoch"], plan["skip"], plan["start_epoch"], plan["rng"], plan["grads"]) == (False, 0, 2, None, None)
    tr._apply_resume(plan, module, tr.runner)
    assert torch.equal(module.model.arena.data, want)
    assert module.optimizer.step_count == 2 and (tr.global_step, tr.runner.global_step, tr.runner.micro_step) == (4, 4, 12)
    assert not module.model.arena.grad.any()
    with pytest.warns(UserWarning, match="no state for the callback EarlyStopping"):
        tr._restore_callbacks(plan, module)


def test_refusals_come_before_the_arena_is_touched(tmp_path):
    _, src, path, _ = _saved(tmp_path)
    good = torch.load(path, weights_only=True)

    def refused(match, edit=None, rank=0, world=1, **kw):
        tr, module = _fresh(tmp_path, **kw)
        a = module.model.arena
        before = {k: getattr(a, k).clone() for k in ("data", "grad", "exp_avg", "exp_avg_sq")}
        ck = torch.load(path, weights_only=True)
        if edit is not None:
            edit(ck)
        bad = str(tmp_path / "bad.ckpt")
        torch.save(ck, bad)
        with pytest.raises(ValueError, match=match):
            tr._plan_resume(bad, module, tr.runner, rank, world)
        assert all(torch.equal(getattr(a, k), v) for k, v in before.items())

    refused("accumulate_grad_batches=3, this run has 4", accumulate=4)
    refused("world size 1, this run has 2", world=2)
    refused("'model.odd' has shape|'odd' has shape",
            lambda ck: ck["state_dict"].update({"model.odd": torch.zeros(3, 33)}))
    refused("no entry for 'table'", lambda ck: ck["state_dict"].pop("model.table"))
    refused("'extra' is not in the model", lambda ck: ck["state_dict"].update({"model.extra": torch.zeros(1)}))
    refused("trainable set: position 1 is 'other' in the file, 'outside' in the model",
            lambda ck: ck[R.RESUME_KEY]["trainable"].__setitem__(1, "other"))
    refused("open-window gradients: no entry for parameter 'q.bias'",
            lambda ck: ck[R.RESUME_KEY]["ranks"][0]["grads"].pop("q.bias"))
    refused("exp_avg: parameter 'odd' has shape",
            lambda ck: ck["optimizer_states"][0]["state"][0].update(exp_avg=torch.zeros(99)))
    assert good["epoch"] == 1


def test_resume_last_without_a_last_checkpoint_is_an_error(tmp_path):
    from sam2_video import train
    cfg = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "overfit_cfg1.json")
    with pytest.raises(FileNotFoundError, match="last.ckpt"):
        train.main(["--config-json", cfg, "--run-dir", str(tmp_path / "run"), "--resume", "last"])
    assert not os.path.exists(tmp_path / "run")  # refused before anything is written
