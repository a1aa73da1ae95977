"""TrainConfig + YAML loader with the reference's field names and parsing behaviour
(ltx_video/config.py:6-154), so configs/train-avatars.yaml drops in unchanged.

Kept quirks (documented, pinned by tests/golden/train_config.json):
  * `precision: "bf16"` stays the string 'bf16' (training.py:30 only reacts to 'bfloat16'); this
    build always computes in bf16 regardless, as BASELINE.json requires.
  * falsy values of rf_shift / rf_target_shift_terminal / rf_log_normal_mu / _sigma become None
    (config.py:125-141): a mu of 0 is read as "unset".
"""
from dataclasses import dataclass
from typing import Optional

import yaml


@dataclass
class TrainConfig:
    checkpoint_path: str
    condition_latents_dir: Optional[str] = None
    encoder_latents_dir: Optional[str] = None
    val_condition_latents_dir: Optional[str] = None
    val_encoder_latents_dir: Optional[str] = None
    videos: Optional[str] = None
    output_dir: Optional[str] = None
    batch_size: Optional[int] = None
    num_epochs: Optional[int] = None
    learning_rate: Optional[float] = None
    lora_rank: int = 8
    lora_alpha: int = 8
    precision: str = "bfloat16"
    gradient_checkpointing: bool = False
    gradient_accumulation_steps: int = 1
    use_deepspeed: bool = False
    deepspeed_config: Optional[str] = None
    local_rank: int = -1
    rf_num_train_timesteps: int = 1000
    rf_sampler: str = "Uniform"
    rf_shift: Optional[float] = None
    rf_shifting: Optional[str] = None
    rf_base_resolution: int = 32 * 32
    rf_target_shift_terminal: Optional[float] = None
    rf_log_normal_mu: Optional[float] = None
    rf_log_normal_sigma: Optional[float] = None
    rf_quantile_min: float = 0.005
    rf_quantile_max: float = 0.999
    wandb_project: str = "ltx-video-avatars"
    wandb_run_name: Optional[str] = None
    log_every_n_steps: int = 10
    save_every_n_epochs: int = 1
    decoder_train: bool = False
    transformer_loss_weight: float = 1.0
    decoder_loss_l1_weight: float = 0.1
    decoder_loss_lpips_weight: float = 0.0
    decoder_t_max: float = 0.1


_SAMPLERS = {"uniform": "Uniform", "linear-quadratic": "LinearQuadratic",
             "linearquadratic": "LinearQuadratic", "from_checkpoint": "Uniform"}


def _opt_float(block, key):
    v = block.get(key)
    return float(v) if v else None


def load_train_config_from_yaml(yaml_path: str) -> TrainConfig:
    with open(yaml_path, "r") as f:
        cfg = yaml.safe_load(f)
    checkpoint_path = cfg.get("checkpoint_path", None)
    if not checkpoint_path:
        raise ValueError("checkpoint_path is required in YAML for training.")
    sampler = cfg.get("sampler", None)
    rf_sampler = _SAMPLERS.get(sampler.lower(), "Uniform") if isinstance(sampler, str) else "Uniform"
    t = cfg.get("train", {}) or {}
    config = TrainConfig(
        checkpoint_path=checkpoint_path,
        precision=cfg.get("precision", "bfloat16"),
        condition_latents_dir=t.get("condition_latents_dir"),
        encoder_latents_dir=t.get("encoder_latents_dir"),
        val_condition_latents_dir=t.get("val_condition_latents_dir"),
        val_encoder_latents_dir=t.get("val_encoder_latents_dir"),
        videos=t.get("videos"),
        output_dir=t.get("output_dir"),
        batch_size=int(t["batch_size"]) if "batch_size" in t else None,
        num_epochs=int(t["num_epochs"]) if "num_epochs" in t else None,
        # `learning_rate: null` reads as unset (Prodigy's 1.0, training.optimizer_from_config)
        learning_rate=float(t["learning_rate"]) if t.get("learning_rate") is not None else None,
        lora_rank=int(t.get("lora_rank", 8)),
        lora_alpha=int(t.get("lora_alpha", 8)),
        gradient_checkpointing=bool(t.get("gradient_checkpointing", False)),
        gradient_accumulation_steps=int(t.get("gradient_accumulation_steps", 1)),
        use_deepspeed=bool(t.get("use_deepspeed", False)),
        deepspeed_config=t.get("deepspeed_config"),
        local_rank=int(t.get("local_rank", -1)),
        rf_sampler=rf_sampler,
        rf_num_train_timesteps=int(t.get("rf_num_train_timesteps", 1000)),
        rf_shift=_opt_float(t, "rf_shift"),
        rf_shifting=t.get("rf_shifting"),
        rf_base_resolution=int(t.get("rf_base_resolution", 32 * 32)),
        rf_target_shift_terminal=_opt_float(t, "rf_target_shift_terminal"),
        rf_log_normal_mu=_opt_float(t, "rf_log_normal_mu"),
        rf_log_normal_sigma=_opt_float(t, "rf_log_normal_sigma"),
        rf_quantile_min=float(t.get("rf_quantile_min", 0.005)),
        rf_quantile_max=float(t.get("rf_quantile_max", 0.999)),
        wandb_project=t.get("wandb_project", "ltx-video-avatars"),
        wandb_run_name=t.get("wandb_run_name"),
        log_every_n_steps=int(t.get("log_every_n_steps", 10)),
        save_every_n_epochs=int(t.get("save_every_n_epochs", 1)),
        decoder_train=bool(t.get("decoder_train", False)),
        transformer_loss_weight=float(t.get("transformer_loss_weight", 1.0)),
        decoder_loss_l1_weight=float(t.get("decoder_loss_l1_weight", 0.1)),
        decoder_loss_lpips_weight=float(t.get("decoder_loss_lpips_weight", 0.0)),
        decoder_t_max=float(t.get("decoder_t_max", 0.1)),
    )
    # this build's extension, not a TrainConfig field (the dataclass stays the reference's): the
    # attentions that carry LoRA adapters, read by lora.apply_training_strategy with getattr, set
    # only when the YAML names it ("attn2", "attn1", "attn1+attn2" or a list of those names)
    if "lora_targets" in t:
        v = t["lora_targets"]
        setattr(config, "lora_targets", v if isinstance(v, str) else tuple(v))
    # likewise `train.lora_ff` (a bool, absent = False): adapters on both feed-forward linears of
    # every block as well (ff.net.0.proj and ff.net.2), with lora_rank / lora_alpha
    if "lora_ff" in t:
        setattr(config, "lora_ff", bool(t["lora_ff"]))
    # and `train.lora_dropout` (a float in [0, 1), absent = 0.0): peft's lora_dropout, one rate for
    # every adapter of the model
    if "lora_dropout" in t:
        setattr(config, "lora_dropout", float(t["lora_dropout"]))
    # and `train.use_dora` (a bool, absent = False): peft's use_dora, weight-decomposed LoRA on the
    # attn2 projections
    if "use_dora" in t:
        setattr(config, "use_dora", bool(t["use_dora"]))
    # and the two keys training.train_loop reads: `train.save_adapters` (a bool, absent = False):
    # <output_dir>/adapter_epoch_{E}/ beside every merged checkpoint; `train.resume_from` (such a
    # directory, or "auto" for the highest complete one in output_dir)
    if "save_adapters" in t:
        setattr(config, "save_adapters", bool(t["save_adapters"]))
    if "resume_from" in t:
        setattr(config, "resume_from", str(t["resume_from"]))
    # and the optimizer-step keys training.schedule_from_config reads (and validates):
    # `train.max_grad_norm` (a float, absent or 0 = no clipping): the global gradient-norm clip of the
    # LoRA step; `train.lr_scheduler` ("constant", "constant_with_warmup", "linear" or "cosine", absent
    # = "constant"), `train.lr_warmup_steps` (absent = 0) and `train.lr_total_steps` (absent = the
    # optimizer steps of the run: num_epochs * (batches per epoch // gradient_accumulation_steps))
    if "max_grad_norm" in t:
        setattr(config, "max_grad_norm", float(t["max_grad_norm"]))
    if "lr_scheduler" in t:
        setattr(config, "lr_scheduler", str(t["lr_scheduler"]))
    if "lr_warmup_steps" in t:
        setattr(config, "lr_warmup_steps", int(t["lr_warmup_steps"]))
    if "lr_total_steps" in t:
        setattr(config, "lr_total_steps", int(t["lr_total_steps"]))
    # and the keys training.ema_from_config reads (and validates): `train.ema_decay` (a float, absent
    # or 0 = no EMA): the exponential moving average of the trained weights inside the LoRA optimizer
    # step, with diffusers' EMAModel schedule: `train.ema_warmup` (a bool), `train.ema_inv_gamma`,
    # `train.ema_power`, `train.ema_update_after_step` and `train.ema_min_decay`
    if "ema_decay" in t:
        setattr(config, "ema_decay", float(t["ema_decay"]))
    if "ema_warmup" in t:
        setattr(config, "ema_warmup", bool(t["ema_warmup"]))
    for key in ("ema_inv_gamma", "ema_power", "ema_min_decay"):
        if key in t:
            setattr(config, key, float(t[key]))
    if "ema_update_after_step" in t:
        setattr(config, "ema_update_after_step", int(t["ema_update_after_step"]))
    # and the keys training.optimizer_from_config reads (and validates): `train.optimizer` ("adamw", the
    # same as absent, or "prodigy": the learning-rate-free optimizer, with `learning_rate: 1.0` or null);
    # `train.weight_decay`, `train.adam_beta1`, `train.adam_beta2`, `train.adam_eps` (absent = the chosen
    # optimizer's defaults); and Prodigy's own `train.prodigy_d0`, `train.prodigy_d_coef`,
    # `train.prodigy_growth_rate`, `train.prodigy_beta3` (floats) and `train.prodigy_use_bias_correction`,
    # `train.prodigy_safeguard_warmup`, `train.prodigy_decouple` (bools)
    if "optimizer" in t:
        setattr(config, "optimizer", str(t["optimizer"]))
    for key in ("weight_decay", "adam_beta1", "adam_beta2", "adam_eps", "prodigy_d0", "prodigy_d_coef",
                "prodigy_growth_rate", "prodigy_beta3"):
        if key in t:
            setattr(config, key, float(t[key]))
    for key in ("prodigy_use_bias_correction", "prodigy_safeguard_warmup", "prodigy_decouple"):
        if key in t:
            setattr(config, key, bool(t[key]))
    # and the two keys of the stochastically rounded bf16 step, read (and validated) there too:
    # `train.bf16_update` ("nearest", the same as absent, or "stochastic": f32 moments and a stochastically
    # rounded store for the bf16 caption projection) and `train.bf16_sr_seed` (an integer in [0, 2^64),
    # absent = 0; the value is passed on as written, so a fraction is refused, not truncated)
    if "bf16_update" in t:
        setattr(config, "bf16_update", str(t["bf16_update"]))
    if "bf16_sr_seed" in t:
        setattr(config, "bf16_sr_seed", t["bf16_sr_seed"])
    # and the two keys training.guard_from_config reads (and validates; the values are passed on as
    # written, so a string or a fraction is refused there): `train.skip_nonfinite` (a bool, absent =
    # false): the optimizer skips, on the device, every step whose gradients are not all finite;
    # `train.max_consecutive_skips` (an integer >= 0, absent or 0 = no limit)
    for key in ("skip_nonfinite", "max_consecutive_skips"):
        if key in t:
            setattr(config, key, t[key])
    # and the four keys training.loss_weights_from_config reads (and validates; passed on as written):
    # `train.loss_face_weight` (a float > 0, absent = 1): the loss weight of the tokens inside the clip's
    # face box; `train.loss_face_pad` (a float >= 0, absent = 0): the box's margin, as a fraction of its
    # size; `train.loss_frame0_weight` (a float >= 0, absent = 1): the weight of the first latent frame;
    # `train.loss_timestep_weighting` ("none", the same as absent, "sigma_sqrt" or "cosmap"). With them
    # `train.face_bbox_dir`: the directory of the preprocessing's {stem}.json files with the `face_bbox`
    # key, the face_bbox_dir argument of io.LatentPairDataset
    for key in ("loss_face_weight", "loss_face_pad", "loss_frame0_weight", "loss_timestep_weighting",
                "face_bbox_dir"):
        if key in t:
            setattr(config, key, t[key])
    # and the three keys training.robust_loss_from_config reads (and validates; passed on as written):
    # `train.loss_type` ("l2", the same as absent, "huber" or "smooth_l1": the pseudo-Huber velocity loss),
    # `train.huber_c` (a float > 0, absent = 0.1: the threshold at t = 1) and `train.huber_schedule`
    # ("constant", "exponential" or "snr", absent = "snr": how the threshold follows the timestep); the
    # last two are refused without a loss_type that reads them
    for key in ("loss_type", "huber_c", "huber_schedule"):
        if key in t:
            setattr(config, key, t[key])
    # and the key training.max_norm_from_config reads (and validates; passed on as written):
    # `train.scale_weight_norms` (a float > 0; absent, null or 0 = off): kohya's max-norm regularisation, the
    # cap on every adapter's |s| ||B A||_F, enforced inside the optimizer step
    if "scale_weight_norms" in t:
        setattr(config, "scale_weight_norms", t["scale_weight_norms"])
    return config
