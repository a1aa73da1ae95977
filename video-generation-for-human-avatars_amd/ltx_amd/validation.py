"""The validation epoch of the reference's train_loop (ltx_video/validation.py:13-95).

validate_epoch keeps the reference's signature and semantics: model.eval(), no_grad, and for each
batch the train step's own draws (LogNormal t with the batch-quantile clamp, then the noise, both
from the device generator) and arithmetic without a backward -- training.train_step(backward=False)
is exactly that pass, through the forward-only kernels (eval launches the p = 0 adapter kernels
whatever lora_dropout is, and draws no dropout key). The result is the mean over batches of
float(bf16 mse); transformer_loss_weight is not applied (validation.py:91). The model is left in
eval mode, as the reference leaves it; train_one_epoch switches back.

validate_video (pipeline, VAE decode, LPIPS / FID) is out of scope.
"""
import torch

from .training import train_step


@torch.no_grad()
def validate_epoch(model, dataloader, scheduler, patchifier, config, prompt_embeds,
                   prompt_attention_mask, device):
    model.eval()
    losses = []
    for batch in dataloader:
        _, _, _, loss_dict = train_step(model, batch, scheduler, patchifier, config, prompt_embeds,
                                        prompt_attention_mask, device, backward=False)
        losses.append(loss_dict["transformer_mse"])  # stays on the device: one host sync below
    total = 0.0
    for mse in losses:
        total += float(mse)
    return total / max(1, len(losses))
