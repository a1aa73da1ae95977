"""The host side of the loss weights, without a GPU: the float64 statement of the token weights
(training.token_loss_weights_ref) on cases worked out by hand, the config keys and their refusals
(training.loss_weights_from_config, the YAML route), the dataset's face boxes, the timestep factors
against their closed forms, and train_step's refusals, which come before anything is launched."""
import json
import math

import pytest
import torch

from loss_weight_utils import closed_form_factor, config, namespace

F64 = torch.float64


def _ref(*a, **k):
    from ltx_amd.training import token_loss_weights_ref
    return token_loss_weights_ref(*a, **k)


def _close(a, b):
    return torch.allclose(a.double(), torch.as_tensor(b, dtype=F64), rtol=1e-12, atol=1e-12)


def test_box_on_cell_edges():
    """F = 3, H = 4, W = 5, box x in [0.2, 0.6], y in [0.25, 0.75]: columns 1-2 and rows 1-2 are covered
    wholly, nothing else. face_weight 4: raw is 4 on 2 x 2 cells of each frame and 1 on the other 16, the
    sum 3 (16 + 16) = 96 over N = 60 tokens, so wt = 4 * 60 / 96 = 2.5 inside and 0.625 outside."""
    box = torch.tensor([[0.2, 0.25, 0.6, 0.75]], dtype=F64)
    wt, raw_sum = _ref(1, 3, 4, 5, bbox=box, face_weight=4.0)
    assert wt.shape == (1, 60) and wt.dtype == F64 and _close(raw_sum, [96.0])
    inside = torch.zeros(3, 4, 5, dtype=torch.bool)
    inside[:, 1:3, 1:3] = True
    want = torch.where(inside, torch.tensor(2.5, dtype=F64), torch.tensor(0.625, dtype=F64)).reshape(1, 60)
    assert _close(wt, want)
    assert _close(wt.mean(dim=1), [1.0])


def test_box_cutting_cells():
    """W = 5, x in [0.3, 0.7] over the whole height: cov = 0, 0.5, 1, 0.5, 0. face_weight 3: raw = 1, 2, 3, 2, 1,
    the sum 9 per row."""
    box = torch.tensor([[0.3, 0.0, 0.7, 1.0]], dtype=F64)
    wt, raw_sum = _ref(1, 1, 1, 5, bbox=box, face_weight=3.0)
    assert _close(raw_sum, [9.0])
    assert _close(wt, [[5 / 9, 10 / 9, 15 / 9, 10 / 9, 5 / 9]])
    # two rows, the box over the lower half of the upper row only: y in [0.25, 0.5] covers half of row 0
    box = torch.tensor([[0.3, 0.25, 0.7, 0.5]], dtype=F64)
    wt, raw_sum = _ref(1, 1, 2, 5, bbox=box, face_weight=3.0)
    raw = torch.tensor([1, 1.5, 2, 1.5, 1, 1, 1, 1, 1, 1], dtype=F64)
    assert _close(raw_sum, [12.0]) and _close(wt, (raw * 10 / 12).reshape(1, 10))


def test_padding_clips_at_the_border():
    """Box (0, 0, 0.4, 0.5) padded by half its size: x in [-0.2, 0.6] -> [0, 0.6], y in [-0.25, 0.75] ->
    [0, 0.75]: columns 0-2 of 5 and rows 0-2 of 4 wholly, 9 cells of 20."""
    box = torch.tensor([[0.0, 0.0, 0.4, 0.5]], dtype=F64)
    wt, raw_sum = _ref(1, 1, 4, 5, bbox=box, face_weight=2.0, face_pad=0.5)
    assert _close(raw_sum, [29.0])
    inside = torch.zeros(4, 5, dtype=torch.bool)
    inside[:3, :3] = True
    want = torch.where(inside, torch.tensor(40 / 29, dtype=F64), torch.tensor(20 / 29, dtype=F64))
    assert _close(wt, want.reshape(1, 20))
    # without the padding only columns 0-1 and rows 0-1
    wt0, raw_sum0 = _ref(1, 1, 4, 5, bbox=box, face_weight=2.0)
    assert _close(raw_sum0, [24.0])
    # a padding that swallows the frame: every cell covered, the weights uniform again
    wt1, _ = _ref(1, 1, 4, 5, bbox=box, face_weight=2.0, face_pad=10.0)
    assert _close(wt1, torch.ones(1, 20))


def test_invalid_boxes_give_uniform_weights():
    nan = float("nan")
    boxes = torch.tensor([[0.2, 0.2, 0.6, 0.6],    # a real box
                          [nan, 0.2, 0.6, 0.6],    # a NaN coordinate
                          [0.6, 0.2, 0.2, 0.6],    # x_max < x_min
                          [0.2, 0.5, 0.6, 0.5],    # no height
                          [1.5, 0.2, 1.9, 0.6],    # outside the frame: empty after the clip
                          [nan, nan, nan, nan]], dtype=F64)
    wt, raw_sum = _ref(6, 2, 5, 5, bbox=boxes, face_weight=4.0, face_pad=0.1)
    assert not _close(wt[0], torch.ones(50)) and not torch.isnan(wt).any()
    assert _close(wt[1:], torch.ones(5, 50)) and _close(raw_sum[1:], torch.full((5,), 50.0))
    # no box at all is the same thing
    wt_none, _ = _ref(6, 2, 5, 5, face_weight=4.0)
    assert _close(wt_none, torch.ones(6, 50))


def test_frame0_weight_zero_and_other_frame_weights():
    fw = torch.tensor([0.0, 1.0, 1.0], dtype=F64)
    wt, raw_sum = _ref(2, 3, 2, 2, frame_w=fw)
    assert _close(raw_sum, [8.0, 8.0])
    assert _close(wt.reshape(2, 3, 4)[:, 0], torch.zeros(2, 4))
    assert _close(wt.reshape(2, 3, 4)[:, 1:], torch.full((2, 2, 4), 1.5))
    # every weight 0: the sample's weights are 0, not NaN
    wt0, raw_sum0 = _ref(1, 1, 2, 2, frame_w=torch.zeros(1, dtype=F64))
    assert _close(raw_sum0, [0.0]) and _close(wt0, torch.zeros(1, 4))


def test_per_sample_mean_is_the_sample_factor():
    g = torch.Generator().manual_seed(3)
    B, F, H, W = 4, 3, 6, 7
    box = torch.tensor([[0.1, 0.2, 0.55, 0.9], [0.3, 0.3, 0.35, 0.35], [float("nan")] * 4, [0.0, 0.0, 1.0, 1.0]])
    sw = torch.rand(B, generator=g) * 3 + 0.1
    uw = torch.rand(B, F, H, W, generator=g)
    fw = torch.rand(F, generator=g)
    wt, raw_sum = _ref(B, F, H, W, bbox=box, frame_w=fw, sample_w=sw, user_w=uw, face_weight=5.0, face_pad=0.2)
    assert wt.shape == (B, F * H * W) and (wt >= 0).all()
    assert torch.allclose(wt.mean(dim=1), sw.double(), rtol=1e-12)
    assert raw_sum.shape == (B,) and (raw_sum > 0).all()
    # [B, N] caller weights are the same thing as [B, F, H, W]
    wt2, _ = _ref(B, F, H, W, bbox=box, frame_w=fw, sample_w=sw, user_w=uw.reshape(B, -1), face_weight=5.0,
                  face_pad=0.2)
    assert torch.equal(wt, wt2)


# ---------------------------------------------------------------------------------------------
# config
# ---------------------------------------------------------------------------------------------
def test_loss_weights_from_config_reads_the_keys():
    from ltx_amd.training import LossWeights, loss_weights_from_config
    assert loss_weights_from_config(config()) is None  # nothing set: the plain loss
    assert loss_weights_from_config(namespace()) is None
    # every key at its default is the plain loss too
    assert loss_weights_from_config(config(loss_face_weight=1.0, loss_face_pad=0.0, loss_frame0_weight=1,
                                           loss_timestep_weighting="none")) is None
    assert loss_weights_from_config(config(loss_face_weight=None, loss_timestep_weighting=None)) is None
    assert loss_weights_from_config(config(loss_face_weight=4)) == LossWeights(4.0, 0.0, 1.0, "none")
    assert loss_weights_from_config(config(loss_face_pad=0.25)) == LossWeights(1.0, 0.25, 1.0, "none")
    assert loss_weights_from_config(config(loss_frame0_weight=0)) == LossWeights(1.0, 0.0, 0.0, "none")
    got = loss_weights_from_config(config(loss_face_weight=0.5, loss_face_pad=0.1, loss_frame0_weight=0.25,
                                          loss_timestep_weighting="cosmap"))
    assert got == LossWeights(0.5, 0.1, 0.25, "cosmap")
    assert loss_weights_from_config(config(loss_timestep_weighting="sigma_sqrt")).timestep_weighting == "sigma_sqrt"


@pytest.mark.parametrize("key,bad", [
    ("loss_face_weight", 0), ("loss_face_weight", -1.0), ("loss_face_weight", float("nan")),
    ("loss_face_weight", float("inf")), ("loss_face_weight", "4"), ("loss_face_weight", True),
    ("loss_face_pad", -0.1), ("loss_face_pad", float("nan")), ("loss_face_pad", "0.1"), ("loss_face_pad", False),
    ("loss_face_pad", float("inf")),
    ("loss_frame0_weight", -1), ("loss_frame0_weight", float("nan")), ("loss_frame0_weight", [1.0]),
    ("loss_frame0_weight", float("inf")),
    ("loss_timestep_weighting", "cosine"), ("loss_timestep_weighting", "COSMAP"), ("loss_timestep_weighting", 1),
    ("loss_timestep_weighting", True), ("loss_timestep_weighting", ""),
])
def test_loss_weights_from_config_refuses(key, bad):
    from ltx_amd.training import loss_weights_from_config
    with pytest.raises(ValueError, match=key):
        loss_weights_from_config(config(**{key: bad}))


def test_yaml_keys_reach_the_config(tmp_path):
    from ltx_amd.config import load_train_config_from_yaml
    from ltx_amd.training import LossWeights, loss_weights_from_config
    plain = tmp_path / "plain.yaml"
    plain.write_text("checkpoint_path: x\ntrain:\n  batch_size: 2\n")
    tc = load_train_config_from_yaml(str(plain))
    for key in ("loss_face_weight", "loss_face_pad", "loss_frame0_weight", "loss_timestep_weighting",
                "face_bbox_dir"):
        assert not hasattr(tc, key), key  # absent keys set nothing
    assert loss_weights_from_config(tc) is None
    full = tmp_path / "full.yaml"
    full.write_text("checkpoint_path: x\ntrain:\n  loss_face_weight: 4\n  loss_face_pad: 0.15\n"
                    "  loss_frame0_weight: 0.25\n  loss_timestep_weighting: cosmap\n  face_bbox_dir: /data/cond\n")
    tc = load_train_config_from_yaml(str(full))
    assert tc.face_bbox_dir == "/data/cond"
    assert loss_weights_from_config(tc) == LossWeights(4.0, 0.15, 0.25, "cosmap")
    # values are passed on as written: a quoted number is refused where it is read, not converted
    bad = tmp_path / "bad.yaml"
    bad.write_text("checkpoint_path: x\ntrain:\n  loss_face_weight: '4'\n")
    with pytest.raises(ValueError, match="loss_face_weight"):
        loss_weights_from_config(load_train_config_from_yaml(str(bad)))


# ---------------------------------------------------------------------------------------------
# timestep factors
# ---------------------------------------------------------------------------------------------
def test_timestep_factors_match_their_closed_forms():
    from ltx_amd.training import timestep_loss_weight
    t = torch.tensor([0.05, 0.25, 0.5, 0.75, 0.95, 0.999], dtype=torch.float32)
    assert timestep_loss_weight(t, "none") is None
    for scheme in ("sigma_sqrt", "cosmap"):
        got = timestep_loss_weight(t, scheme)
        assert got.dtype == torch.float32 and got.shape == t.shape and got.is_contiguous()
        # a handful of f32 roundings on values of order 1: 1e-6 relative is generous by a factor of ten
        assert torch.allclose(got.double(), closed_form_factor(t, scheme), rtol=1e-6, atol=0)
    # the values themselves: t^-2 at 0.5 is 4; cosmap peaks at t = 0.5 with 4 / pi and is 2 / pi at the ends
    assert float(timestep_loss_weight(torch.tensor([0.5]), "sigma_sqrt")) == 4.0
    cos = timestep_loss_weight(torch.tensor([0.0, 0.5, 1.0]), "cosmap").double()
    assert torch.allclose(cos, torch.tensor([2 / math.pi, 4 / math.pi, 2 / math.pi], dtype=F64), rtol=1e-6)
    with pytest.raises(ValueError, match="loss_timestep_weighting"):
        timestep_loss_weight(t, "snr")


# ---------------------------------------------------------------------------------------------
# dataset
# ---------------------------------------------------------------------------------------------
def _write_clip(cond, enc, stem, F=2, H=4, W=4):
    from ltx_amd import io
    io.save_latents_pt(torch.randn(1, 128, F, H, W), enc / f"{stem}.pt")
    io.save_latents_pt(torch.randn(1, 128, F, H, W), cond / f"{stem}.pt")
    io.save_latents_pt(torch.randn(1, 128, 1, H, W), cond / f"{stem}_ref.pt")


def test_dataset_reads_face_boxes(tmp_path):
    from ltx_amd import io
    cond, enc, meta = tmp_path / "cond", tmp_path / "enc", tmp_path / "meta"
    for p in (cond, enc, meta):
        p.mkdir()
    for stem in ("a_0", "b_0", "c_0", "d_0", "e_0"):
        _write_clip(cond, enc, stem)
    # the preprocessing's file: the box as a dict of the four names, among the clip's other metadata
    (meta / "a_0.json").write_text(json.dumps({"video": "a", "clip_index": 0, "fps": 25.0, "face_bbox": {
        "x_min": 0.25, "y_min": 0.125, "x_max": 0.75, "y_max": 0.5}, "format": "conditioning_data"}))
    (meta / "b_0.json").write_text(json.dumps({"face_bbox": {"x_min": 0.1, "y_min": 0.2, "x_max": 0.3, "y_max": 0.4}}))
    (meta / "c_0.json").write_text(json.dumps({"video": "c"}))  # the key is missing
    (meta / "d_0.json").write_text("{ not json")                # d: unreadable; e: no file at all
    ds = io.LatentPairDataset(str(cond), str(enc), face_bbox_dir=str(meta))
    assert len(ds) == 5
    items = [ds[i] for i in range(5)]
    assert [it["stem"] for it in items] == ["a_0", "b_0", "c_0", "d_0", "e_0"]
    for it in items:
        assert set(it) == {"latents", "pose_latents", "ref_image_latents", "stem", "face_bbox"}
        assert it["face_bbox"].dtype == torch.float32 and it["face_bbox"].shape == (4,)
    assert items[0]["face_bbox"].tolist() == [0.25, 0.125, 0.75, 0.5]
    assert torch.equal(items[1]["face_bbox"], torch.tensor([0.1, 0.2, 0.3, 0.4]))
    for it in items[2:]:
        assert torch.isnan(it["face_bbox"]).all()
    batch = io.collate_latent_pairs(items[:3])
    assert batch["face_bbox"].shape == (3, 4) and batch["face_bbox"].dtype == torch.float32
    assert torch.equal(batch["face_bbox"][0], items[0]["face_bbox"]) and torch.isnan(batch["face_bbox"][2]).all()
    # the condition directory itself may hold the JSON files
    (cond / "a_0.json").write_text(json.dumps({"face_bbox": {"x_min": 0, "y_min": 0, "x_max": 1, "y_max": 1}}))
    assert io.LatentPairDataset(str(cond), str(enc), face_bbox_dir=str(cond))[0]["face_bbox"].tolist() == [0, 0, 1, 1]
    # the loader keeps the box f32 while the latents go to bf16
    loader = io.LatentLoader(ds, 2, "cpu", shuffle=False)
    first = next(iter(loader))
    assert first["face_bbox"].dtype == torch.float32 and first["latents"].dtype == torch.bfloat16
    assert torch.equal(first["face_bbox"][0], items[0]["face_bbox"])


def test_dataset_without_face_bbox_dir_is_unchanged(tmp_path):
    from ltx_amd import io
    cond, enc = tmp_path / "cond", tmp_path / "enc"
    cond.mkdir()
    enc.mkdir()
    _write_clip(cond, enc, "a_0")
    (cond / "a_0.json").write_text(json.dumps({"face_bbox": {"x_min": 0.1, "y_min": 0.2, "x_max": 0.3, "y_max": 0.4}}))
    ds = io.LatentPairDataset(str(cond), str(enc))
    assert set(ds[0]) == {"latents", "pose_latents", "ref_image_latents", "stem"}
    assert set(io.collate_latent_pairs([ds[0]])) == {"latents", "pose_latents", "ref_image_latents", "stem"}
    assert set(next(iter(io.LatentLoader(ds, 1, "cpu", shuffle=False)))) == {"latents", "pose_latents",
                                                                              "ref_image_latents", "stem"}


# ---------------------------------------------------------------------------------------------
# train_step's refusals: raised from the shapes alone, before the model or a kernel is touched
# ---------------------------------------------------------------------------------------------
def _cpu_batch(F):
    return {"latents": torch.zeros(2, 128, F, 4, 4), "ref_image_latents": torch.zeros(2, 128, 1, 4, 4),
            "pose_latents": torch.zeros(2, 128, F, 4, 4)}


def test_train_step_refuses_frame0_zero_with_one_frame():
    from ltx_amd.training import train_step
    tc = config(loss_frame0_weight=0.0)
    with pytest.raises(ValueError, match="loss_frame0_weight"):
        train_step(None, _cpu_batch(1), None, None, tc, None, None, device="cpu")


def test_train_step_refuses_misshapen_loss_weights():
    from ltx_amd.training import train_step
    batch = dict(_cpu_batch(2), loss_weights=torch.ones(2, 2, 4))
    with pytest.raises(ValueError, match="loss_weights"):
        train_step(None, batch, None, None, config(), None, None, device="cpu")
    with pytest.raises(ValueError, match="loss_face_pad"):
        train_step(None, _cpu_batch(2), None, None, config(loss_face_pad=-1.0), None, None, device="cpu")
