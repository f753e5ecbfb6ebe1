"""Trainer.fit(ckpt_path=...) on the device: a resumed run against the uninterrupted one, bit for bit.

Every fit runs in a spawned child process of its own (a real resume is a fresh process, and one process keeps to
one fit), reports through a queue and leaves its tensors in a file; a child that fails, dies or runs out of time
fails the fixture, and nothing further is started.

Layout (the smallest at which every restored item can go wrong): tests/golden/overfit_cfg1.json (Hiera-T 256^2),
2-frame synthetic clips, 4 train clips shuffled, bf16, captured step graph, dropout as configured, 2 positive + 1
negative random clicks (the host generator), accumulate_grad_batches 3, a validation every 2 batches, 1 sanity
validation step, max_epochs 3, ModelCheckpoint(save_top_k=-1, save_last=True).  Every epoch then has a validation
with an open window of 2 micro-steps, a full window, a validation with an open window of 1, and the one-batch
flush: 2 optimizer steps per epoch, checkpoints epoch=e-step=2e and epoch=e-step=2e+1.

Seconds per case on an MI355X are in DESIGN.md §9 (each child builds the model and captures the step graph)."""
import copy
import json
import os
import shutil
import socket
import time

import pytest
import torch
import torch.multiprocessing as mp

from step_harness import GOLD

pytestmark = pytest.mark.gpu

CFG = os.path.join(GOLD, "overfit_cfg1.json")
HERE = os.path.dirname(os.path.abspath(__file__))
CHILD_LIMIT = 300  # seconds; a child normally takes a small fraction of it
_FAILED = []


def _sections(trainable=None):
    with open(CFG) as f:
        cfg = copy.deepcopy(json.load(f))
    for model in (cfg["model"], cfg["module"]["model"]):
        model.update(use_activation_checkpoint=False, num_pos_points=2, num_neg_points=1)
        if trainable is not None:
            model["trainable_modules"] = list(trainable)
    for data in (cfg["data"], cfg["data_module"]["data"]):
        data.update(video_clip_length=2, num_workers=0, synthetic_clips=4)
    cfg["data_module"]["train_shuffle"] = True
    return cfg


def _seed(seed):
    import random

    import numpy as np
    torch.manual_seed(seed)
    random.seed(seed)
    np.random.seed(seed)


class Snapshot:
    """what the foreign-file case looks at between the load and the first step"""

    def __init__(self):
        self.seen = None

    def on_fit_start(self, trainer, pl_module):
        from sam2_video.kernels import ops
        arena, opt = pl_module.model.arena, pl_module.optimizer
        self.seen = {"data": arena.data.cpu().clone(), "exp_avg": arena.exp_avg.cpu().clone(),
                     "exp_avg_sq": arena.exp_avg_sq.cpu().clone(), "step_count": opt.step_count,
                     "lr": opt.param_groups[0]["lr"], "global_step": trainer.global_step,
                     "shadow_is_cast": torch.equal(arena.shadow, ops.cast(arena.data, torch.bfloat16)),
                     "grad_zero": not bool(arena.grad.any())}


def _foreign_file(cfg, path):
    """a Lightning / reference checkpoint built on the host: the model's state_dict with the `model.` prefix and
    a real torch AdamW over the reference's parameter list, stepped twice on synthetic gradients (none for the
    parameters the step never reaches, as in the reference, where their .grad stays None)"""
    from sam2_video.model.build import instantiate
    src = instantiate(cfg["model"])
    never = set(src.never_grad_parameter_names())
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():
        for p in src.parameters():
            p.add_(0.01 * torch.randn(p.shape, generator=g))
    named = [(n, p) for n, p in src.named_parameters() if p.requires_grad]
    opt = torch.optim.AdamW([p for _, p in named], lr=5e-5, betas=(0.9, 0.999), weight_decay=0.01)
    for _ in range(2):
        for n, p in named:
            p.grad = None if n in never else 0.01 * torch.randn(p.shape, generator=g)
        opt.step()
    torch.save({"state_dict": {"model." + k: v.detach().clone() for k, v in src.state_dict().items()},
                "optimizer_states": [opt.state_dict()], "global_step": 2, "epoch": 0,
                "lr_schedulers": [], "callbacks": {}}, path)
    want = {"params": {n: p.detach().clone() for n, p in src.named_parameters()},
            "exp_avg": {n: opt.state[p]["exp_avg"].clone() for n, p in named if p in opt.state},
            "exp_avg_sq": {n: opt.state[p]["exp_avg_sq"].clone() for n, p in named if p in opt.state}}
    return want


def _child(spec, q):
    """one fit; spec: root, out, kind (fit | foreign | mismatch | complete), swa, max_epochs, ckpt_path, seed, rank,
    world, port, save_after (fit: write <root>/final.ckpt after the fit, as train.main does)"""
    rank = spec.get("rank", 0)
    try:
        import sys
        import warnings
        for p in (HERE, os.path.join(os.path.dirname(HERE), "sam2-video-training_amd")):
            if p not in sys.path:
                sys.path.insert(0, p)
        world = spec.get("world", 1)
        if world > 1:
            os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(spec["port"]), RANK=str(rank),
                              WORLD_SIZE=str(world), LOCAL_RANK="0")  # both ranks share the one GPU
            from sam2_video.training.ddp import init_from_env
            init_from_env("gloo")
        torch.cuda.set_device(0)
        from sam2_video.model.build import instantiate
        from sam2_video.training import callbacks as C
        from sam2_video.training.trainer import Trainer
        kind = spec.get("kind", "fit")
        cfg = _sections(["memory_attention"] if kind == "mismatch" else None)
        _seed(spec.get("seed", 42))
        module = instantiate(cfg["module"], _recursive_=False)
        dm = instantiate(cfg["data_module"], _recursive_=False)
        root = spec["root"]
        ck = C.ModelCheckpoint(save_top_k=-1, save_last=True, dirpath=os.path.join(root, "checkpoints"))
        cbs = [ck]
        if spec.get("swa"):
            cbs.append(C.StochasticWeightAveraging(swa_lrs=0.005, swa_epoch_start=0.67, annealing_epochs=1))
        kw = dict(max_epochs=spec.get("max_epochs", 3), precision=16, gradient_clip_val=1.0, accumulate_grad_batches=3,
                  val_check_interval=2, limit_val_batches=1, num_sanity_val_steps=1, log_every_n_steps=1, graph=True,
                  callbacks=cbs, default_root_dir=os.path.join(root, "logs"))
        ckpt_path = spec.get("ckpt_path")
        out = {}
        t0 = time.time()
        if kind == "mismatch":
            dev = torch.device("cuda", 0)
            module.compute_dtype = "bf16"
            module.setup("fit", dev)
            before = module.model.arena.data.cpu().clone()
            try:
                Trainer(**kw).fit(module, dm, ckpt_path=ckpt_path)
                out["raised"] = None
            except ValueError as e:
                out["raised"] = str(e)
            arena = module.model.arena
            out["unchanged"] = bool(torch.equal(arena.data.cpu(), before) and not arena.exp_avg.any()
                                    and not arena.exp_avg_sq.any() and not arena.grad.any()
                                    and module.optimizer.step_count == 0)
        elif kind == "foreign":
            ckpt_path = os.path.join(root, "foreign.ckpt")
            os.makedirs(root, exist_ok=True)
            out["want"] = _foreign_file(cfg, ckpt_path)
            snap = Snapshot()
            kw.update(max_epochs=1, max_steps=3, limit_train_batches=1, limit_val_batches=0, accumulate_grad_batches=1,
                      num_sanity_val_steps=0, callbacks=[snap])  # the file is at global_step 2: one step is left
            trainer = Trainer(**kw)
            with warnings.catch_warnings(record=True) as caught:
                warnings.simplefilter("always")
                trainer.fit(module, dm, ckpt_path=ckpt_path)
            torch.cuda.synchronize()
            arena = module.model.arena
            out.update(seen=snap.seen, warnings=[str(w.message) for w in caught if "ckpt_path" in str(w.message)],
                       offsets={n: (arena.offsets[n], arena.params[n].numel()) for n in arena.order},
                       grad_names=list(arena.grad_names), step_count=module.optimizer.step_count,
                       global_step=trainer.global_step, data_after=arena.data.cpu().clone(),
                       loss=[row["train/total_loss"] for row in trainer.history])
        else:
            trainer = Trainer(**kw)
            with warnings.catch_warnings(record=True) as caught:
                warnings.simplefilter("always")
                trainer.fit(module, dm, ckpt_path=ckpt_path)
            out["warnings"] = [str(w.message) for w in caught if "ckpt_path" in str(w.message)]
            torch.cuda.synchronize()
            if spec.get("save_after"):
                trainer.save_checkpoint(os.path.join(root, "final.ckpt"))
            arena = module.model.arena
            n = arena.n_grad
            files = sorted(os.path.relpath(os.path.join(d, f), ck.dirpath) for d, _, fs in os.walk(ck.dirpath) for f in fs)
            out.update(history=trainer.history, val_history=trainer.val_history, data=arena.data[:n].cpu().clone(),
                       data_all=arena.data.cpu().clone(), exp_avg=arena.exp_avg.cpu().clone(),
                       exp_avg_sq=arena.exp_avg_sq.cpu().clone(), shadow=arena.shadow[:n].cpu().clone(),
                       shadow_all=arena.shadow.cpu().clone(), checkpoint_state=ck.state_dict(), files=files,
                       global_step=trainer.global_step, step_count=module.optimizer.step_count,
                       graphs=len(trainer.runner._graphs), metrics=dict(trainer.callback_metrics),
                       swa=[(cb.n_averaged, cb.swa_start, cb.swa_end, cb.applied) for cb in cbs[1:]])
        out["seconds"] = time.time() - t0
        torch.save(out, spec["out"])
        q.put((rank, True, out["seconds"]))
    except Exception:  # pragma: no cover - reported to the parent
        import traceback
        q.put((rank, False, traceback.format_exc()))
    finally:
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            dist.destroy_process_group()


def _run_children(specs):
    """starts one process per spec (more than one: the ranks of one run), waits for every report; returns the
    saved results.  Fails -- and bars every later start -- when a child reports failure, dies or takes too long."""
    if _FAILED:
        pytest.fail("not started: an earlier child process failed (%s)" % _FAILED[0][:200])
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_child, args=(s, q)) for s in specs]
    for p in procs:
        p.start()
    reports, deadline = [], time.time() + CHILD_LIMIT
    problem = None
    while len(reports) < len(procs) and problem is None:
        try:
            reports.append(q.get(timeout=1.0))
            if not reports[-1][1]:
                problem = "child reported: %s" % reports[-1][2]
        except Exception:  # queue.Empty
            if time.time() > deadline:
                problem = "child ran longer than %d s" % CHILD_LIMIT
            elif any(not p.is_alive() and p.exitcode != 0 for p in procs):
                problem = "child died with exit code %s" % [p.exitcode for p in procs]
    for p in procs:
        p.join(timeout=5 if problem else 60)
        if p.is_alive():
            p.kill()
    if problem is not None:
        _FAILED.append(problem)
        pytest.fail(problem)
    return [torch.load(s["out"], map_location="cpu", weights_only=False) for s in specs]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _killed_after(root, keep):
    """the checkpoint directory as a job killed right after writing `keep[-1]` left it"""
    ckdir = os.path.join(root, "checkpoints")
    for f in os.listdir(ckdir):
        if f not in keep and f != "last.ckpt":
            os.remove(os.path.join(ckdir, f))


def _pair(tmp, name, resume_from, keep, **kw):
    """(straight, resumed): the straight run, then -- in the same directories, with the files written after
    `resume_from` removed -- a run resumed from a copy of the straight run's own `resume_from`, seeded differently"""
    root = str(tmp / name)
    world = kw.get("world", 1)
    port = _free_port()
    straight = _run_children([dict(kw, root=root, out=str(tmp / f"{name}_straight{r}.pt"), seed=42, rank=r, port=port)
                              for r in range(world)])
    ckpt = str(tmp / f"{name}_resume.ckpt")
    shutil.copy(os.path.join(root, "checkpoints", resume_from), ckpt)
    _killed_after(root, keep)
    port = _free_port()
    resumed = _run_children([dict(kw, root=root, out=str(tmp / f"{name}_resumed{r}.pt"), seed=977 + r, rank=r,
                                  port=port, ckpt_path=ckpt) for r in range(world)])
    return straight, resumed, ckpt


def _names(epochs):
    return sorted([f"epoch={e}-step={2 * e + k}.ckpt" for e in range(epochs) for k in (0, 1)] + ["last.ckpt"])


def _rows(rows):
    return [{k: v for k, v in r.items() if k != "time_s"} for r in rows]


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("resume_plain")
    # epoch 1's first validation: 2 micro-steps of a window of 3 are in the gradient arena
    s, r, ckpt = _pair(tmp, "plain", "epoch=1-step=2.ckpt", ["epoch=0-step=0.ckpt", "epoch=0-step=1.ckpt", "epoch=1-step=2.ckpt"])
    return {"straight": s[0], "resumed": r[0], "ckpt": ckpt}


def test_the_checkpoint_was_taken_with_a_window_open(plain):
    from sam2_video.training import resume as R
    ck = torch.load(plain["ckpt"], map_location="cpu", weights_only=True)
    b = ck[R.RESUME_KEY]
    assert (ck["epoch"], ck["global_step"], b["micro_step"], b["accumulate"], b["batches_done"]) == (1, 2, 8, 3, 2)
    assert b["epoch_finished"] is False and b["world_size"] == 1
    grads = b["ranks"][0]["grads"]
    assert grads and any(bool(g.any()) for g in grads.values())
    s = plain["straight"]
    assert s["files"] == _names(3) and s["global_step"] == 6 and s["step_count"] == 6
    # (a history row is written for the steps taken inside the batch loop: each epoch's full window, not its flush)
    assert [row["step"] for row in s["history"]] == [1, 3, 5] and len(s["val_history"]) == 6 and 1 <= s["graphs"] <= 2


def test_resumed_run_reproduces_the_histories(plain):
    s, r = plain["straight"], plain["resumed"]
    assert _rows(r["history"]) == _rows(s["history"])
    assert _rows(r["val_history"]) == _rows(s["val_history"])
    assert r["metrics"] == s["metrics"] and r["global_step"] == s["global_step"] and r["step_count"] == s["step_count"]
    losses = [row["train/total_loss"] for row in s["history"]]
    assert len(set(losses)) == len(losses)  # (the steps differ: equal rows are no accident)


def test_resumed_run_reproduces_the_final_tensors_bit_for_bit(plain):
    s, r = plain["straight"], plain["resumed"]
    for name in ("data", "exp_avg", "exp_avg_sq", "shadow", "data_all", "shadow_all"):
        assert torch.equal(r[name], s[name]), name
    assert bool(s["exp_avg"].any())


def test_resumed_run_writes_the_same_checkpoint_files(plain):
    s, r = plain["straight"], plain["resumed"]
    assert r["files"] == s["files"] == _names(3)
    assert r["checkpoint_state"] == s["checkpoint_state"]
    assert os.path.basename(r["checkpoint_state"]["best_model_path"]) == "epoch=2-step=5.ckpt"


@pytest.fixture(scope="module")
def swa(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("resume_swa")
    # swa_start = int(3 * 0.67) - 1 = 1: the first swa_update runs at the start of epoch 1, before this checkpoint
    s, r, ckpt = _pair(tmp, "swa", "epoch=1-step=2.ckpt", ["epoch=0-step=0.ckpt", "epoch=0-step=1.ckpt", "epoch=1-step=2.ckpt"],
                       swa=True)
    return {"straight": s[0], "resumed": r[0], "ckpt": ckpt}


def test_swa_average_and_schedule_survive_the_resume(swa):
    from sam2_video.training import resume as R
    ck = torch.load(swa["ckpt"], map_location="cpu", weights_only=True)
    state = ck["callbacks"]["StochasticWeightAveraging"]
    assert (state["n_averaged"], state["_latest_update_epoch"], state["applied"]) == (1, 1, False)
    assert state["schedule"] is not None and ck[R.RESUME_KEY]["swa"] and ck[R.RESUME_KEY]["lr_override"] is not None
    s, r = swa["straight"], swa["resumed"]
    assert s["swa"] == r["swa"] == [(2, 1, 2, True)]
    for name in ("data_all", "shadow_all", "exp_avg", "exp_avg_sq"):  # the master after swa_apply, and its shadow
        assert torch.equal(r[name], s[name]), name
    assert _rows(r["history"]) == _rows(s["history"]) and _rows(r["val_history"]) == _rows(s["val_history"])
    assert [row["train/learning_rate"] for row in s["history"]][-1] == 0.005


@pytest.fixture(scope="module")
def two_ranks(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("resume_ddp")
    # 2 clips per rank and epoch: the validation after batch 2 finds a window of 2 open on each rank (each rank's
    # own, unreduced partial sums), then the flush reduces and steps
    s, r, ckpt = _pair(tmp, "ddp", "epoch=1-step=1.ckpt", ["epoch=0-step=0.ckpt", "epoch=1-step=1.ckpt"],
                       world=2, max_epochs=2)
    return {"straight": s, "resumed": r, "ckpt": ckpt}


def test_two_ranks_resume_to_the_same_arena(two_ranks):
    from sam2_video.training import resume as R
    b = torch.load(two_ranks["ckpt"], map_location="cpu", weights_only=True)[R.RESUME_KEY]
    assert b["world_size"] == 2 and len(b["ranks"]) == 2 and b["micro_step"] % 3 == 2
    g0, g1 = b["ranks"][0]["grads"], b["ranks"][1]["grads"]
    assert any(not torch.equal(g0[n], g1[n]) for n in g0)  # each rank's own partial sums
    s, r = two_ranks["straight"], two_ranks["resumed"]
    for name in ("data_all", "shadow_all", "exp_avg", "exp_avg_sq"):
        assert torch.equal(s[0][name], s[1][name]), name
        assert torch.equal(r[0][name], r[1][name]), name
        assert torch.equal(r[0][name], s[0][name]), name
    assert r[0]["global_step"] == s[0]["global_step"] == 2
    assert r[0]["files"] == s[0]["files"] == sorted(["epoch=0-step=0.ckpt", "epoch=1-step=1.ckpt", "last.ckpt"])


@pytest.fixture(scope="module")
def foreign(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("resume_foreign")
    return _run_children([dict(kind="foreign", root=str(tmp / "run"), out=str(tmp / "foreign.pt"))])[0]


def test_a_foreign_checkpoint_resumes(foreign):
    want, seen = foreign["want"], foreign["seen"]
    assert len(foreign["warnings"]) == 1 and "position inside epoch 0 is not known" in foreign["warnings"][0]
    assert seen["step_count"] == 2 and seen["lr"] == 5e-5 and seen["global_step"] == 2
    assert seen["shadow_is_cast"] and seen["grad_zero"]
    assert sorted(want["exp_avg"]) == sorted(foreign["grad_names"])
    for n, (o, numel) in foreign["offsets"].items():
        assert torch.equal(seen["data"][o:o + numel], want["params"][n].reshape(-1)), n
    covered = torch.zeros(seen["exp_avg"].numel(), dtype=torch.bool)
    for n in foreign["grad_names"]:
        o, numel = foreign["offsets"][n]
        covered[o:o + numel] = True
        assert torch.equal(seen["exp_avg"][o:o + numel], want["exp_avg"][n].reshape(-1)), n
        assert torch.equal(seen["exp_avg_sq"][o:o + numel], want["exp_avg_sq"][n].reshape(-1)), n
    assert not seen["exp_avg"][~covered].any() and not seen["exp_avg_sq"][~covered].any()
    # one training step ran on top of it
    assert foreign["step_count"] == 3 and foreign["global_step"] == 3 and len(foreign["loss"]) == 1
    assert not torch.equal(foreign["data_after"], seen["data"]) and bool(torch.isfinite(foreign["data_after"]).all())


def test_a_mismatched_trainable_set_is_refused_before_the_arena_is_touched(plain, tmp_path):
    got = _run_children([dict(kind="mismatch", root=str(tmp_path / "run"), out=str(tmp_path / "mismatch.pt"),
                              ckpt_path=plain["ckpt"])])[0]
    assert got["raised"] is not None and "trainable set" in got["raised"] and "memory_encoder" in got["raised"]
    assert got["unchanged"]


@pytest.fixture(scope="module")
def finished(tmp_path_factory):
    """a one-epoch run that writes a checkpoint after its fit, and a fit given that checkpoint"""
    tmp = tmp_path_factory.mktemp("resume_finished")
    root = str(tmp / "run")
    first = _run_children([dict(root=root, out=str(tmp / "first.pt"), max_epochs=1, save_after=True)])[0]
    again = _run_children([dict(root=root, out=str(tmp / "again.pt"), max_epochs=1, seed=5,
                                ckpt_path=os.path.join(root, "final.ckpt"))])[0]
    return first, again


def test_a_finished_run_trains_nothing_and_says_so_once(finished):
    first, again = finished
    assert first["warnings"] == [] and first["global_step"] == 2
    assert len(again["warnings"]) == 1 and "complete" in again["warnings"][0] and "nothing is trained" in again["warnings"][0]
    assert again["graphs"] == 0 and again["global_step"] == 2 and again["step_count"] == 2
    assert _rows(again["history"]) == _rows(first["history"]) and again["history"] == first["history"]
    assert again["val_history"] == first["val_history"] and again["files"] == first["files"]
    for name in ("data_all", "shadow_all", "exp_avg", "exp_avg_sq"):
        assert torch.equal(again[name], first[name]), name
