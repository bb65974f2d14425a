"""What the SD1.5 sampler (generation.py) and the SDXL sampler (generation_sdxl.py) share below their public surface: the reference's
numeric helpers, the DDIM grid and its endpoint rule, the bounded cache of per-step device constants, the boundary step on the fused
HIP kernel, the w-embedding, and the `editing` / `cond_only` contexts.  The four loops stay in the two modules - their UNet calls differ
(CFG doubling and dead-uncond elimination there, added_cond_kwargs and the amplify prompt here) - and call what is in this file.
"""
import contextlib

import numpy as np
import torch

from . import p2p


# ----------------------------------------------------------------------------------------------------------- numeric helpers
def linear_schedule_old(t, guidance_scale, tau1, tau2):
    """gamma(t/1000) * gs with gamma = 1 below tau1, 0 above tau2, linear in between (utils/generation.py:74-82).
    `guidance_scale` is a float on the SD1.5 path and a one-element tensor on the SDXL path (utils/generation_sdxl.py:439-440)."""
    u = t / 1000
    if u <= tau1:
        gamma = 1.0
    elif u >= tau2:
        gamma = 0.0
    else:
        gamma = (tau2 - u) / (tau2 - tau1)
    return gamma * guidance_scale


def guidance_scale_embedding(w, embedding_dim=512, dtype=torch.float32):
    """[sin(1000 w f) || cos(1000 w f)], f_i = exp(-ln(1e4) i / (half - 1))  (utils/generation.py:96-122, generation_sdxl.py:84-110)."""
    assert len(w.shape) == 1
    w = w * 1000.0
    half_dim = embedding_dim // 2
    step = torch.log(torch.tensor(10000.0)) / (half_dim - 1)
    freqs = torch.exp(torch.arange(half_dim, dtype=dtype) * -step)
    ang = w.to(dtype)[:, None] * freqs[None, :]
    emb = torch.cat([torch.sin(ang), torch.cos(ang)], dim=1)
    if embedding_dim % 2 == 1:
        emb = torch.nn.functional.pad(emb, (0, 1))
    assert emb.shape == (w.shape[0], embedding_dim)
    return emb


def extract_into_tensor(a, t, x_shape):
    b, *_ = t.shape
    return a.gather(-1, t).reshape(b, *((1,) * (len(x_shape) - 1)))


def predicted_origin(model_output, timesteps, boundary_timesteps, sample, prediction_type, alphas, sigmas):
    """x0-prediction followed by the jump to the boundary timestep s (utils/generation.py:136-155, generation_sdxl.py:112-132).

    Generic torch expression (any device); the sampler loops use the fused HIP kernel icd_x0_step (boundary_step below), which is
    bit-identical to this expression evaluated in fp32."""
    sigmas_s = extract_into_tensor(sigmas, boundary_timesteps, sample.shape)
    alphas_s = extract_into_tensor(alphas, boundary_timesteps, sample.shape)
    sigmas_t = extract_into_tensor(sigmas, timesteps, sample.shape)
    alphas_t = extract_into_tensor(alphas, timesteps, sample.shape)
    alphas_s[boundary_timesteps == 0] = 1.0          # hard boundary at s = 0
    sigmas_s[boundary_timesteps == 0] = 0.0
    if prediction_type == "epsilon":
        x0 = (sample - sigmas_t * model_output) / alphas_t
        return alphas_s * x0 + sigmas_s * model_output
    if prediction_type == "v_prediction":
        assert boundary_timesteps == 0, "v_prediction does not support multiple endpoints at the moment"
        return alphas_t * sample - sigmas_t * model_output
    raise ValueError(f"Prediction type {prediction_type} currently not supported.")


# ----------------------------------------------------------------------------------------------------------- timestep tables
def ddim_grid(n_steps, n_train=1000):
    """The DDIM timesteps of both samplers as a numpy int64 array: 19, 39, ..., 999 for 50 steps of 1000."""
    return (np.arange(1, n_steps + 1) * (n_train // n_steps)).round().astype(np.int64) - 1


def interval_endpoints(ddim_timesteps, num_endpoints, max_inverse_timestep_index):
    """(endpoints, inverse endpoints) of a consistency model with `num_endpoints` boundaries on the grid `ddim_timesteps` (a CPU long
    tensor): utils/generation.py:453-465 and DDIMSolver, utils/generation_sdxl.py:160-174, are this one rule."""
    n = len(ddim_timesteps)
    step = n // num_endpoints + int(n % num_endpoints > 0)
    idx = torch.arange(step, n, step) - 1
    inv_idx = torch.tensor(idx.tolist() + [max_inverse_timestep_index])
    return torch.tensor([0] + ddim_timesteps[idx].tolist()), ddim_timesteps[inv_idx]


def schedules(scheduler):
    """(alpha, sigma) tables of the boundary step on the host"""
    ac = scheduler.alphas_cumprod
    return torch.sqrt(ac).cpu(), torch.sqrt(1 - ac).cpu()


# ----------------------------------------------------------------------------------------------------------- contexts
def editing(model, on):
    """`with unet.editing():` when `on` and the UNet of the model / pipeline is the native one (anything else: no-op)."""
    ctx = getattr(getattr(model, "unet", None), "editing", None)
    return ctx() if (on and ctx is not None) else contextlib.nullcontext()


@contextlib.contextmanager
def cond_only(unet, on=True):
    """Every row the UNet sees inside is a conditional one (the executor's cond-only hook layout); the previous value comes back."""
    if not on:
        yield
        return
    prev, unet.attn_cond_only = unet.attn_cond_only, True
    try:
        yield
    finally:
        unet.attn_cond_only = prev


# ----------------------------------------------------------------------------------------------------------- device constants
class ConstCache:
    """Per-step constants on the device (w-embeddings, boundary coefficients), so that a loop that has run once issues no host->device
    copy and never synchronises.  At most LIMIT entries: the one that would exceed it empties the cache first."""
    LIMIT = 256

    def __init__(self):
        self.entries = {}

    def get(self, key, make):
        v = self.entries.get(key)
        if v is None:
            if len(self.entries) >= self.LIMIT:
                self.entries.clear()
            v = self.entries[key] = make()
        return v


def w_embedding(values, dim, device, dtype, cache):
    values = tuple(map(float, values))
    return cache.get(("w", values, dim, str(device), dtype),
                     lambda: guidance_scale_embedding(torch.tensor(values), embedding_dim=dim).to(device=device, dtype=dtype))


# ----------------------------------------------------------------------------------------------------------- boundary step
def boundary_coefficients(t, s, alpha_schedule, sigma_schedule):
    """(alpha_t, sigma_t, alpha_s, sigma_s) of predicted_origin as Python floats, with the hard boundary (1, 0) at s = 0."""
    a_s, s_s = (1.0, 0.0) if s == 0 else (float(alpha_schedule[s]), float(sigma_schedule[s]))
    return float(alpha_schedule[t]), float(sigma_schedule[t]), a_s, s_s


def coefficient_rows(t, s, batch, device, alpha_schedule, sigma_schedule, cache):
    """The [batch, 4] fp32 operand of icd_x0_step.  The key carries the schedule's value at t: a cache may outlive a scheduler."""
    key = ("coef", t, s, batch, str(device), float(alpha_schedule[t]))
    return cache.get(key, lambda: torch.tensor([boundary_coefficients(t, s, alpha_schedule, sigma_schedule)] * batch,
                                               dtype=torch.float32).to(device))


def boundary_step(noise_pred, t, s, latents, prediction_type, alpha_schedule, sigma_schedule, out_dtype, cache):
    """predicted_origin for a whole batch at one (t, s) pair, as `out_dtype` - the fused HIP kernel on the GPU."""
    B = len(latents)
    if latents.is_cuda and prediction_type == "epsilon":
        from . import ops
        coef = coefficient_rows(int(t), int(s), B, latents.device, alpha_schedule, sigma_schedule, cache)
        return ops.x0_step(latents.contiguous(), noise_pred.contiguous(), coef, out_dtype=out_dtype)
    dev = latents.device
    return predicted_origin(noise_pred, torch.tensor([t] * B, device=dev), torch.tensor([s] * B, device=dev), latents,
                            prediction_type, alpha_schedule.to(dev), sigma_schedule.to(dev)).to(out_dtype)


# ----------------------------------------------------------------------------------------------------------- prompt groups
def prompt_groups(prompt, controller):
    """(G, P) for a list of G lists of P prompts (batched editing), None for the reference's flat list."""
    if isinstance(prompt, str) or not any(isinstance(p, (list, tuple)) for p in prompt):
        return None
    if not all(isinstance(p, (list, tuple)) and len(p) > 0 for p in prompt):
        raise ValueError("runner: a prompt list mixes groups (lists) and single prompts")
    sizes = {len(p) for p in prompt}
    if len(sizes) != 1:
        raise ValueError(f"runner: every prompt group must have the same size (got {sorted(sizes)}); split the batch by size")
    G, P = len(prompt), sizes.pop()
    if controller is not None:
        if not isinstance(controller, p2p.ControllerBatch):
            raise ValueError("runner: grouped prompts need a p2p.ControllerBatch (one controller per group)")
        if controller.n_groups != G or (controller.is_edit and controller.n_prompts != P):
            raise ValueError(f"runner: {G} groups of {P} prompts do not match the ControllerBatch "
                             f"({controller.n_groups} members of {controller.n_prompts} prompts)")
    return G, P


def expand_edit_latents(latents, batch_size, groups):
    """Latents of an edit: one sample for all prompts (init_latent of the SD1.5 runner), one per prompt group, or one per prompt."""
    n = latents.shape[0]
    if n == batch_size:
        return latents
    if n == 1:
        return latents.expand(batch_size, *latents.shape[1:]).contiguous()
    if groups is not None and n == groups[0]:
        return latents.repeat_interleave(groups[1], 0)
    raise ValueError(f"sample_deterministic: {n} latents for {batch_size} prompts"
                     + ("" if groups is None else f" in {groups[0]} groups of {groups[1]}"))
