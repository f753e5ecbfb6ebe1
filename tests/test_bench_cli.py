"""bench.py's command line and its output dump, without a GPU: a plain run keeps every leg beyond the
timed steps off, --full switches them on (and the single-leg switches still work under it), the
options that read the profiled step ask for --full, and --dump-outputs writes float32 arrays, large
ones as the same seeded sample on every call."""
import importlib.util
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _parse(bench, monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_has_every_extra_leg_off(bench, monkeypatch):
    a = _parse(bench, monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    assert a.no_trace and a.no_prof and a.cpu_baseline == 0
    a = _parse(bench, monkeypatch, "--steps", "3", "--dump-outputs", "d")
    assert a.dump_outputs == "d" and a.no_prof


def test_full_run_keeps_the_legs_and_their_switches(bench, monkeypatch):
    a = _parse(bench, monkeypatch, "--full")
    assert a.full and not a.no_trace and not a.no_prof and a.cpu_baseline == 1
    a = _parse(bench, monkeypatch, "--full", "--no-trace", "--cpu-baseline", "0", "--kernel-table")
    assert a.no_trace and not a.no_prof and a.cpu_baseline == 0 and a.kernel_table


@pytest.mark.parametrize("argv", [("--kernel-table",), ("--shape-table", "t.txt"), ("--trace-out", "t.csv"),
                                  ("--steps", "0")])
def test_rejected_arguments(bench, monkeypatch, argv):
    with pytest.raises(SystemExit) as e:
        _parse(bench, monkeypatch, *argv)
    assert e.value.code == 2


@pytest.mark.parametrize("numel", [(1 << 18) + 1, 3 * (1 << 18) + 7, 1 << 25, 80_000_003])
def test_sample_indices_are_distinct_in_range_and_repeatable(bench, numel):
    idx = bench.sample_indices(numel)
    assert idx.shape == (bench.DUMP_SAMPLE,) and idx.dtype == np.int64
    assert idx[0] >= 0 and idx[-1] < numel and (np.diff(idx) > 0).all()
    assert np.array_equal(idx, bench.sample_indices(numel))


def test_dump_outputs_writes_float32_and_samples_large_arrays(bench, tmp_path):
    n = bench.DUMP_SAMPLE
    g = torch.Generator().manual_seed(0)
    data = torch.randn(3 * n, generator=g, dtype=torch.float64)
    grad = torch.randn(2 * n + 5, generator=g)
    masks = [torch.randn(4, 1, 8, 8, generator=g) for _ in range(3)]
    arena = types.SimpleNamespace(data=data, grad_region=lambda: grad)
    # a second name of one tensor is written once; a tensor shared by all frames still gives a row per frame
    shared = torch.ones(2)
    frames = [{"pred_masks": m, "multistep_pred_masks": m, "shared": shared, "multistep_pred_ious": [m[:, :, 0, 0].to(torch.bfloat16)],
               "multistep_point_inputs": [None], "ragged": torch.ones(t + 1)} for t, m in enumerate(masks)]
    module = types.SimpleNamespace(logged={"train/total_loss": torch.tensor(1.5), "train/learning_rate": 1e-6},
                                   last_outputs=frames, model=types.SimpleNamespace(arena=arena))
    out = [tmp_path / "a", tmp_path / "b"]
    for d in out:
        bench.dump_outputs(str(d), torch.tensor(1.5), module)
    got = {f[:-4]: np.load(out[0] / f) for f in sorted(os.listdir(out[0]))}
    assert sorted(got) == ["frame0_ragged", "frame1_ragged", "frame2_ragged", "frames_multistep_pred_ious",
                           "frames_pred_masks", "frames_shared", "grad_arena", "logged_train_total_loss", "loss", "param_arena"]
    assert all(a.dtype == np.float32 for a in got.values())
    assert got["loss"].shape == () and float(got["loss"]) == 1.5
    assert np.array_equal(got["frames_pred_masks"], torch.stack(masks).numpy())  # small: whole, shape kept
    assert got["frames_multistep_pred_ious"].shape == (3, 4, 1) and got["frames_shared"].shape == (3, 2)
    assert got["param_arena"].shape == (n,) and got["grad_arena"].shape == (n,)
    assert np.isin(got["param_arena"], data.float().numpy()).all()  # a sample of the array's own elements
    for f in os.listdir(out[0]):  # the same elements on every call
        assert np.array_equal(np.load(out[0] / f), np.load(out[1] / f))
    assert sum(a.nbytes for a in got.values()) <= 64 * 10**6
