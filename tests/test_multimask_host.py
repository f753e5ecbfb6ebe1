"""The three-mask SAM heads' host side (no GPU): when they apply (`_use_multimask`), how the flags reach
the model (`model_overrides`, YAML configs, build_sam2_video_predictor's table) and that a training
forward with them is refused."""
import pytest
import torch
import yaml

FLAGS = {"multimask_output_in_sam": True, "multimask_output_for_tracking": True,
         "use_multimask_token_for_obj_ptr": True, "multimask_min_pt_num": 0, "multimask_max_pt_num": 1}
STABILITY = {"dynamic_multimask_via_stability": True, "dynamic_multimask_stability_delta": 0.05,
             "dynamic_multimask_stability_thresh": 0.98}


def _model(**overrides):
    from sam2_video.model.sam2model import SAM2Model
    return SAM2Model(None, "tiny@128", trainable_modules=[], model_overrides=overrides or None)


def _points(n):
    return None if n is None else {"point_coords": torch.zeros(1, n, 2), "point_labels": torch.ones(1, n, dtype=torch.int32)}


def test_use_multimask_truth_table():
    """reference sam2_base.py:932-940: the flag, (init cond frame or tracking flag), min <= points <= max;
    a box is two points, a tracked frame without prompt has none"""
    m = _model(**FLAGS)
    # upstream's released flags (min 0, max 1): a tracked frame and one click yes, a box / two clicks no
    assert m._use_multimask(False, None) is True
    assert m._use_multimask(True, _points(1)) is True
    assert m._use_multimask(False, _points(1)) is True
    assert m._use_multimask(True, _points(2)) is False
    assert m._use_multimask(True, _points(3)) is False
    # without multimask_output_for_tracking only initial conditioning frames qualify
    m = _model(**{**FLAGS, "multimask_output_for_tracking": False})
    assert m._use_multimask(True, _points(1)) is True
    assert m._use_multimask(False, _points(1)) is False
    assert m._use_multimask(False, None) is False
    # min 1: a frame without points does not qualify; max 2 admits a box
    m = _model(**{**FLAGS, "multimask_min_pt_num": 1, "multimask_max_pt_num": 2})
    assert m._use_multimask(False, None) is False
    assert m._use_multimask(True, _points(2)) is True
    assert m._use_multimask(True, _points(3)) is False
    # the flag off: never
    m = _model()
    for init in (True, False):
        for n in (None, 1, 2):
            assert m._use_multimask(init, _points(n)) is False


def test_model_overrides_merge():
    from sam2_video.model.sam2model import merge_model_overrides
    cfg = {"a": 1, "multimask_output_in_sam": False, "sam_mask_decoder_extra_args": {"x": 1, "y": 2}}
    out = merge_model_overrides(cfg, {"multimask_output_in_sam": True, "sam_mask_decoder_extra_args": {"y": 3, "z": 4}})
    assert out == {"a": 1, "multimask_output_in_sam": True, "sam_mask_decoder_extra_args": {"x": 1, "y": 3, "z": 4}}
    assert cfg["sam_mask_decoder_extra_args"] == {"x": 1, "y": 2} and cfg["multimask_output_in_sam"] is False
    assert merge_model_overrides(cfg, None) == cfg
    assert merge_model_overrides({"a": 1}, {"sam_mask_decoder_extra_args": {"z": 4}}) == \
        {"a": 1, "sam_mask_decoder_extra_args": {"z": 4}}
    # through the constructor: the decoder stores what the reference's decoder stores
    m = _model(**FLAGS, sam_mask_decoder_extra_args=dict(STABILITY, dynamic_multimask_stability_thresh=0.9))
    d = m.sam_mask_decoder
    assert m.multimask_output_in_sam and m.multimask_output_for_tracking and m.use_multimask_token_for_obj_ptr
    assert (m.multimask_min_pt_num, m.multimask_max_pt_num) == (0, 1) and d.use_multimask_token_for_obj_ptr
    assert d.dynamic_multimask_via_stability is True
    assert (d.dynamic_multimask_stability_delta, d.dynamic_multimask_stability_thresh) == (0.05, 0.9)
    plain = _model().sam_mask_decoder
    assert plain.dynamic_multimask_via_stability is False
    # overriding changes no parameter: same state_dict keys and synthetic weights
    a, b = _model().state_dict(), m.state_dict()
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)


def test_upstream_overrides_table():
    """what build_sam2_video_predictor(multimask=True) applies: the five flags of upstream's released
    configs and the three decoder arguments upstream's builder adds"""
    from sam2_video.predictor import UPSTREAM_MULTIMASK_OVERRIDES as U
    assert {k: v for k, v in U.items() if k != "sam_mask_decoder_extra_args"} == FLAGS
    assert U["sam_mask_decoder_extra_args"] == STABILITY


def test_yaml_with_multimask_flags_loads(tmp_path):
    from sam2_video.model.configs import model_config
    from sam2_video.model.sam2model import SAM2Model
    cfg = model_config("tiny", 128)
    cfg.update(FLAGS)
    cfg["sam_mask_decoder_extra_args"] = dict(STABILITY)
    path = tmp_path / "sam2.1_hiera_t_multimask.yaml"
    path.write_text(yaml.safe_dump({"model": cfg}))
    m = SAM2Model(None, str(path), trainable_modules=[])
    assert m.multimask_output_in_sam and m.sam_mask_decoder.dynamic_multimask_via_stability
    assert m._use_multimask(False, None) is True


def test_training_forward_with_multimask_flags_is_refused():
    from sam2_video.data.synthetic import synthetic_batch
    m = _model(**FLAGS)
    m.train()
    batch = synthetic_batch(0, 2, 128, 3, 2)
    with pytest.raises(NotImplementedError, match="inference only") as e:
        m(batch)
    assert "multimask_output_in_sam" in str(e.value) and "eval()" in str(e.value)
    with pytest.raises(NotImplementedError, match="inference only"):
        m.forward_tracking({}, batch)
