"""The predictor's hole filling on the device against the host scipy path, end to end: Hiera-T at 256^2,
bf16, three objects (click, box, mask) prompted on a middle frame, tracked in reverse then forward with
fill_hole_area=8.  Every yielded mask and every bank entry must be equal bit for bit."""
import pytest
import torch

from step_harness import build_model

pytestmark = pytest.mark.gpu


def _run(model, frames, pts, labs, on_device):
    from sam2_video import predictor as P
    S, T = 256, frames.shape[0]
    changed = [0]
    real_dev, real_host = P.fill_holes_in_mask_scores, P._fill_holes_host

    def count(fn):
        def wrapped(mask, max_area):
            out = fn(mask, max_area)
            changed[0] += int((out != mask).sum().item())
            return out
        return wrapped

    # count what the fill changes (test-side wrapper around whichever path runs)
    P.fill_holes_in_mask_scores, P._fill_holes_host = count(real_dev), count(real_host)
    try:
        pred = P.SAM2VideoPredictor(model, fill_hole_area=8, postprocess_on_device=on_device)
        st = pred.init_state(frames)
        mid = 2
        out = {}
        _, _, out[("p", "click")] = pred.add_new_points_or_box(st, mid, obj_id=1, points=pts, labels=labs)
        _, _, out[("p", "box")] = pred.add_new_points_or_box(st, mid, obj_id=2, box=[10, 20, 120, 140])
        mask = torch.zeros(S, S, dtype=torch.bool)
        mask[40:100, 60:150] = True
        _, ids, out[("p", "mask")] = pred.add_new_mask(st, mid, obj_id=3, mask=mask)
        assert ids == [1, 2, 3]
        out = {k: v.clone() for k, v in out.items()}
        for t, _, vm in pred.propagate_in_video(st, reverse=True):
            out[("r", t)] = vm.clone()
        for t, _, vm in pred.propagate_in_video(st):
            out[("f", t)] = vm.clone()
        assert sorted(t for d, t in out if d == "r") == list(range(mid + 1))
        assert sorted(t for d, t in out if d == "f") == list(range(mid, T))
        bank = {}
        for i, d in st["output_dict_per_obj"].items():
            for key in ("cond_frame_outputs", "non_cond_frame_outputs"):
                for t, e in d[key].items():
                    for name in ("pred_masks", "maskmem_features", "obj_ptr"):
                        bank[(i, key, t, name)] = e[name].clone()
    finally:
        P.fill_holes_in_mask_scores, P._fill_holes_host = real_dev, real_host
    return out, bank, changed[0]


def test_device_postprocessing_equals_host_path():
    S, T = 256, 4
    model = build_model("tiny", S, [], "point", dtype="bf16", seed=3)
    frames = (torch.rand(T, S, S, 3, generator=torch.Generator().manual_seed(0)) * 255).to(torch.uint8).numpy()
    pts, labs = [[100.0, 90.0]], [1]
    dev_out, dev_bank, dev_changed = _run(model, frames, pts, labs, True)
    host_out, host_bank, host_changed = _run(model, frames, pts, labs, False)
    print(f"low-res pixels changed by the fill over the run: device {dev_changed}, host {host_changed}")
    assert set(dev_out) == set(host_out) and set(dev_bank) == set(host_bank)
    assert len(dev_bank) == 3 * T * 3
    for k in dev_out:
        assert torch.equal(dev_out[k], host_out[k]), f"yielded masks differ at {k}"
    for k in dev_bank:
        assert dev_bank[k].is_cuda and torch.equal(dev_bank[k], host_bank[k]), f"bank entries differ at {k}"


def test_default_path_does_not_leave_the_device(monkeypatch):
    """with the knob at its default a tracked frame's post-processing makes no host copy: the scipy
    labelling is never reached"""
    from sam2_video import predictor as P

    def boom(*a, **k):
        raise AssertionError("host scipy reached on the default per-frame path")

    monkeypatch.setattr(P, "_connected_components", boom)
    S, T = 256, 2
    model = build_model("tiny", S, [], "point", dtype="bf16", seed=3)
    frames = (torch.rand(T, S, S, 3, generator=torch.Generator().manual_seed(1)) * 255).to(torch.uint8).numpy()
    pred = P.SAM2VideoPredictor(model, fill_hole_area=8)
    assert pred.postprocess_on_device
    st = pred.init_state(frames)
    pred.add_new_points_or_box(st, 0, obj_id=1, points=[[100.0, 90.0]], labels=[1])
    assert [t for t, _, _ in pred.propagate_in_video(st)] == [0, 1]
