"""SD1.5 iCD sampler / inverter on the native MI355X UNet (API mirror of the reference's utils/generation.py).

Drop-in surface kept: `runner(...)`, `Generator(...)` with `cons_generation`, `cons_inversion`, `get_noise_pred`,
`init_prompt`, `image2latent`, `latent2image`, `ddim_loop`, `ddim_inversion`, `prev_step`, `next_step`, and the helpers
`linear_schedule_old`, `linear_schedule`, `guidance_scale_embedding`, `extract_into_tensor`, `predicted_origin`,
`guided_step`, `latent2image`, `init_latent`, `load_512`.  Semantics (including the reference's quirks, SURVEY.md
section 8a rows a1-a8) are pinned by golden vectors captured from the reference (tests/test_generation_golden.py).

What is different underneath (MI355X-first):
  * the UNet call is one native executor call (no per-op Python), the boundary step is one fused HIP kernel;
  * when `w_embed_dim > 0` the reference computes the CFG-doubled batch and throws the unconditional half away
    (utils/generation.py:245-251).  `Generator.eliminate_dead_uncond` (default True) evaluates the conditional half
    only - identical outputs, half the FLOPs; controllers still see exactly the rows their `forward` saw before;
  * per-step device constants (w-embedding, timestep, boundary coefficients) are cached on the GPU, so the 4-step loop
    issues no host->device copies and never synchronises (the reference syncs at t.item() every step).
Everything the loops share with the SDXL sampler (the numeric helpers, the endpoint rule, the constant cache, the boundary step) is
sampling.py's.
"""
import numpy as np
import torch

from . import p2p, sampling
from .sampling import extract_into_tensor, guidance_scale_embedding, linear_schedule_old, predicted_origin  # noqa: F401  (drop-in names)


# ----------------------------------------------------------------------------------------------------------- runner
@torch.no_grad()
def runner(model, prompt, controller, solver, is_cons_forward=False, num_inference_steps=50, guidance_scale=7.5,
           generator=None, latent=None, uncond_embeddings=None, start_time=50, return_type='image',
           dynamic_guidance=False, tau1=0.4, tau2=0.6, w_embed_dim=0):
    """utils/generation.py:12-66.  Returns (image | latents, the [1,4,64,64] initial latent).

    Batched editing: `prompt` may be a list of G lists of P prompts (one image's [source, edit_1, ...] each) with a
    p2p.ControllerBatch of G members and `latent` [G, 4, 64, 64] (or None: G draws from `generator` in one call).  Each group's
    latent is repeated P times (init_latent per group), per-step `uncond_embeddings` [G, 77, 768] are repeated per group, and the
    G * P outputs come back group-major, each group as a run of its own would give it.  Returns (images | latents, [G, 4, 64, 64])."""
    groups = sampling.prompt_groups(prompt, controller)
    p2p.register_attention_control(model, controller)
    if groups is None:
        solver.init_prompt(prompt, None)
        latent, latents = init_latent(latent, model, 512, 512, generator, len(prompt))      # resolution is fixed, :32-34
    else:
        G, P = groups
        solver.init_prompt([p for grp in prompt for p in grp], None)
        latent, latents = init_latent_groups(latent, model, 512, 512, generator, G, P)
        if uncond_embeddings is not None:
            uncond_embeddings = [u.repeat_interleave(P, 0) if u.shape[0] == G else u for u in uncond_embeddings]
    model.scheduler.set_timesteps(num_inference_steps)
    dynamic_guidance = tau1 < 1.0                      # the argument is overridden and tau2 is never looked at (:36)
    prev_groups, solver.prompt_groups = getattr(solver, "prompt_groups", None), groups
    try:
        if is_cons_forward:
            trajectory = solver.cons_generation(latents, guidance_scale=guidance_scale, w_embed_dim=w_embed_dim,
                                                dynamic_guidance=dynamic_guidance, tau1=tau1, tau2=tau2, controller=controller)
        else:
            trajectory = solver.ddim_loop(latents, num_inference_steps, is_forward=False, guidance_scale=guidance_scale,
                                          dynamic_guidance=dynamic_guidance, tau1=tau1, tau2=tau2, w_embed_dim=w_embed_dim,
                                          uncond_embeddings=uncond_embeddings, controller=controller)
    finally:
        solver.prompt_groups = prev_groups
    latents = trajectory[-1]
    if return_type == 'image':
        image = latent2image(model.vae, latents.to(model.vae.dtype))
    elif return_type == 'uint8_device':                # the same bytes, left on the device (metrics.py scores them there)
        image = latent2image(model.vae, latents.to(model.vae.dtype), on_device=True)
    else:
        image = latents
    return image, latent


# ----------------------------------------------------------------------------------------------------------- schedules
def linear_schedule(t, guidance_scale, tau1=0.4, tau2=0.8):
    """Classic-CFG variant: gs below tau1, 1.0 above tau2 (utils/generation.py:85-93)."""
    u = t / 1000
    if u <= tau1:
        return guidance_scale
    if u >= tau2:
        return 1.0
    return (tau2 - u) / (tau2 - tau1) * (guidance_scale - 1.0) + 1.0


def guided_step(noise_prediction_text, noise_pred_uncond, t, guidance_scale, dynamic_guidance=False, tau1=0.4, tau2=0.6):
    if dynamic_guidance:
        if not isinstance(t, int):
            t = t.item()
        guidance_scale = linear_schedule(t, guidance_scale, tau1=tau1, tau2=tau2)
    return noise_pred_uncond + guidance_scale * (noise_prediction_text - noise_pred_uncond)


# ----------------------------------------------------------------------------------------------------------- Generator
class Generator:
    """Few-step consistency sampler / inverter (utils/generation.py:181-521)."""

    eliminate_dead_uncond = True     # skip the unconditional CFG rows when their output is discarded (w_embed_dim > 0)
    prompt_groups = None             # (G, P) while a batch of G independent prompt groups runs (runner / cons_inversion)

    def __init__(self, model, n_steps, noise_scheduler, forward_cons_model=None, reverse_cons_model=None, num_endpoints=1,
                 num_forward_endpoints=1, reverse_timesteps=None, forward_timesteps=None, max_forward_timestep_index=49,
                 start_timestep=19):
        self.model = model
        self.forward_cons_model = forward_cons_model
        self.reverse_cons_model = reverse_cons_model
        self.noise_scheduler = noise_scheduler
        self.n_steps = n_steps
        self.tokenizer = self.model.tokenizer
        self.model.scheduler.set_timesteps(n_steps)
        self.prompt = None
        self.context = None
        self.ddim_timesteps = torch.from_numpy(sampling.ddim_grid(n_steps)).long()
        self.start_timestep = start_timestep
        self._consts = sampling.ConstCache()     # per Generator: the schedules of its models

        if reverse_timesteps is None or forward_timesteps is None:
            ends, inv_ends = self._create_forward_inverse_timesteps(num_endpoints, n_steps, max_forward_timestep_index)
            self.reverse_timesteps, self.reverse_boundary_timesteps = inv_ends.flip(0), ends.flip(0)
            ends, inv_ends = self._create_forward_inverse_timesteps(num_forward_endpoints, n_steps, max_forward_timestep_index)
            self.forward_timesteps, self.forward_boundary_timesteps = ends, inv_ends
            self.forward_timesteps[0] = self.start_timestep
        else:
            # the reference reverses the CALLER's list in place (utils/generation.py:507-508); kept for drop-in parity
            reverse_timesteps.reverse()
            rev_boundary = reverse_timesteps[1:] + [0]
            fwd_boundary = forward_timesteps[1:] + [999]
            self.reverse_timesteps = torch.tensor(reverse_timesteps)
            self.reverse_boundary_timesteps = torch.tensor(rev_boundary)
            self.forward_timesteps = torch.tensor(forward_timesteps)
            self.forward_boundary_timesteps = torch.tensor(fwd_boundary)
        print(f"Endpoints reverse CTM: {self.reverse_timesteps}, {self.reverse_boundary_timesteps}")
        print(f"Endpoints forward CTM: {self.forward_timesteps}, {self.forward_boundary_timesteps}")

    def _create_forward_inverse_timesteps(self, num_endpoints, n_steps, max_inverse_timestep_index):
        assert n_steps == len(self.ddim_timesteps)
        return sampling.interval_endpoints(self.ddim_timesteps, num_endpoints, max_inverse_timestep_index)

    @property
    def scheduler(self):
        return self.model.scheduler

    # ------------------------------------------------------------------ DDIM baselines (utils/generation.py:183-205)
    def prev_step(self, model_output, timestep: int, sample):
        prev_t = timestep - self.scheduler.config.num_train_timesteps // self.scheduler.num_inference_steps
        a_t = self.scheduler.alphas_cumprod[timestep]
        a_prev = self.scheduler.alphas_cumprod[prev_t] if prev_t >= 0 else self.scheduler.final_alpha_cumprod
        x0 = (sample - (1 - a_t) ** 0.5 * model_output) / a_t ** 0.5
        return a_prev ** 0.5 * x0 + (1 - a_prev) ** 0.5 * model_output

    def next_step(self, model_output, timestep: int, sample):
        timestep, next_t = min(timestep - self.scheduler.config.num_train_timesteps // self.scheduler.num_inference_steps,
                               999), timestep
        a_t = self.scheduler.alphas_cumprod[timestep] if timestep >= 0 else self.scheduler.final_alpha_cumprod
        a_next = self.scheduler.alphas_cumprod[next_t]
        x0 = (sample - (1 - a_t) ** 0.5 * model_output) / a_t ** 0.5
        return a_next ** 0.5 * x0 + (1 - a_next) ** 0.5 * model_output

    def get_noise_pred_single(self, latents, t, context):
        return self.model.unet(latents, t, encoder_hidden_states=context)["sample"]

    # ------------------------------------------------------------------ the UNet call (utils/generation.py:211-253)
    def _w_vector(self, n_doubled, guidance_scale):
        # [0, 0, 0, gs] iff the CFG-doubled batch is exactly 4, else gs everywhere (utils/generation.py:232-235)
        groups = self.prompt_groups
        if groups is not None and groups[0] * groups[1] * 2 == n_doubled:
            # per group, as each group's run of its own would build it: [uncond of every group ; cond of every group]
            one = self._w_vector_single(2 * groups[1], guidance_scale)
            return one[:groups[1]] * groups[0] + one[groups[1]:] * groups[0]
        return self._w_vector_single(n_doubled, guidance_scale)

    @staticmethod
    def _w_vector_single(n_doubled, guidance_scale):
        if n_doubled == 4:
            return (0.0, 0.0, 0.0, float(guidance_scale))
        return (float(guidance_scale),) * n_doubled

    def _can_skip_uncond(self, model):
        unet = model.unet
        if not (self.eliminate_dead_uncond and hasattr(unet, "attn_cond_only")):
            return False
        ctrl = getattr(unet, "attn_controller", None)
        return ctrl is None or isinstance(ctrl, (p2p.AttentionControl, p2p.EmptyControl))

    def get_noise_pred(self, model, latent, t, guidance_scale=1, context=None, w_embed_dim=0, dynamic_guidance=False,
                       tau1=0.4, tau2=0.6):
        if context is None:
            context = self.context
        B = len(latent)
        w_embedding = None
        if w_embed_dim > 0:
            if dynamic_guidance:
                t_item = t if isinstance(t, int) else t.item()
                guidance_scale = linear_schedule_old(t_item, guidance_scale, tau1=tau1, tau2=tau2)
            w_embedding = sampling.w_embedding(self._w_vector(2 * B, guidance_scale), w_embed_dim, latent.device, latent.dtype,
                                               self._consts)
        unet = model.unet
        if w_embedding is not None and self._can_skip_uncond(model):
            # the unconditional half is dead code on this branch (only `noise_prediction_text` is returned): skip it
            with sampling.cond_only(unet):
                return unet(latent.to(dtype=unet.dtype), t, timestep_cond=w_embedding[B:].to(dtype=unet.dtype),
                            encoder_hidden_states=context[B:])["sample"]
        latents_input = torch.cat([latent] * 2)
        noise_pred = unet(latents_input.to(dtype=unet.dtype), t,
                          timestep_cond=w_embedding.to(dtype=unet.dtype) if w_embed_dim > 0 else None,
                          encoder_hidden_states=context)["sample"]
        noise_pred_uncond, noise_prediction_text = noise_pred.chunk(2)
        if guidance_scale > 1 and w_embedding is None:
            return guided_step(noise_prediction_text, noise_pred_uncond, t, guidance_scale, dynamic_guidance, tau1, tau2)
        return noise_prediction_text

    # ------------------------------------------------------------------ VAE / text plumbing (out of the hot path)
    @torch.no_grad()
    def latent2image(self, latents, return_type='np'):
        """'np': the FIRST image as a uint8 HWC array (utils/generation.py); 'uint8_device': the whole batch, uint8 NHWC on the device."""
        latents = 1 / 0.18215 * latents.detach()
        image = self.model.vae.decode(latents.to(dtype=self.model.dtype))['sample']
        if return_type == 'np':
            image = _to_uint8_host(image[:1])[0]
        elif return_type == 'uint8_device':
            image = _to_uint8_device(image)
        return image

    @torch.no_grad()
    def image2latent(self, image, return_bytes=False):
        """A floating-point 4-d tensor is a latent already.  A uint8 [B, H, W, 3] tensor on the device, or a list of uint8 [H, W, 3]
        device tensors of any sizes (load_512(..., device=)), is resized to 512 x 512 like load_512 and encoded without leaving the
        device (vae.encode_images); return_bytes: (latent, the resized uint8 [B, 512, 512, 3]).  numpy / PIL images take the
        reference's host route."""
        if _is_device_images(image):
            enc = self.model.vae.encode_images(image, 512, want_bytes=return_bytes)
            latent = enc['latent_dist'].mean * 0.18215
            return (latent, enc['images']) if return_bytes else latent
        if return_bytes:
            raise ValueError("image2latent: return_bytes needs uint8 images on the device")
        if type(image) is torch.Tensor and image.dim() == 4:
            return image
        if type(image) is list:
            arr = np.concatenate([np.array(i).reshape(1, 512, 512, 3) for i in image])
            x = (torch.from_numpy(arr).float() / 127.5 - 1).permute(0, 3, 1, 2)
            x = x.to(self.model.device, dtype=self.model.vae.dtype)
        else:
            x = (torch.from_numpy(np.array(image)).float() / 127.5 - 1).permute(2, 0, 1).unsqueeze(0)
            x = x.to(self.model.device, dtype=self.model.dtype)
        return self.model.vae.encode(x)['latent_dist'].mean * 0.18215

    @torch.no_grad()
    def init_prompt(self, prompt, uncond_embeddings=None):
        tok = self.model.tokenizer
        if uncond_embeddings is None:
            ids = tok([""], padding="max_length", max_length=tok.model_max_length, return_tensors="pt").input_ids
            uncond_embeddings = self.model.text_encoder(ids.to(self.model.device))[0]
        ids = tok(prompt, padding="max_length", max_length=tok.model_max_length, truncation=True, return_tensors="pt").input_ids
        text_embeddings = self.model.text_encoder(ids.to(self.model.device))[0]
        self.context = torch.cat([uncond_embeddings.expand(*text_embeddings.shape), text_embeddings])
        self.prompt = prompt

    # ------------------------------------------------------------------ DDIM loops (baselines)
    @torch.no_grad()
    def ddim_loop(self, latent, n_steps, is_forward=True, guidance_scale=1, dynamic_guidance=False, tau1=0.4, tau2=0.6,
                  w_embed_dim=0, uncond_embeddings=None, controller=None):
        all_latent = [latent]
        latent = latent.clone().detach()
        ts = self.model.scheduler.timesteps
        with sampling.editing(self.model, is_forward or dynamic_guidance):
            for i in range(n_steps):
                if uncond_embeddings is not None:
                    self.init_prompt(self.prompt, uncond_embeddings[i])
                t = ts[len(ts) - i - 1] if is_forward else ts[i]
                noise_pred = self.get_noise_pred(model=self.model, latent=latent, t=t, context=None, guidance_scale=guidance_scale,
                                                 dynamic_guidance=dynamic_guidance, w_embed_dim=w_embed_dim, tau1=tau1, tau2=tau2)
                latent = self.next_step(noise_pred, t, latent) if is_forward else self.prev_step(noise_pred, t, latent)
                if controller is not None:
                    latent = controller.step_callback(latent)
                all_latent.append(latent)
        return all_latent

    @torch.no_grad()
    def ddim_inversion(self, image, n_steps=None, guidance_scale=1, dynamic_guidance=False, tau1=0.4, tau2=0.6, w_embed_dim=0,
                       device_images=False):
        """device_images (uint8 images on the device): image_rec is the pair (the images at 512 x 512, the whole decoded batch), both
        uint8 NHWC on the device."""
        n_steps = self.n_steps if n_steps is None else n_steps
        if device_images:
            latent, image_gt = self.image2latent(image, return_bytes=True)
            image_rec = (image_gt, self.latent2image(latent, return_type='uint8_device'))
        else:
            latent = self.image2latent(image)
            image_rec = self.latent2image(latent)
        return image_rec, self.ddim_loop(latent, is_forward=True, guidance_scale=guidance_scale, n_steps=n_steps,
                                         dynamic_guidance=dynamic_guidance, tau1=tau1, tau2=tau2, w_embed_dim=w_embed_dim)

    # ------------------------------------------------------------------ consistency loops (THE hot path)
    def _boundary_step(self, noise_pred, t, s, latent, alpha_schedule, sigma_schedule):
        """sampling.boundary_step with the fp32 latent chain of the reference: the dtype predicted_origin gives on fp32 tables."""
        out_dtype = torch.promote_types(torch.promote_types(latent.dtype, noise_pred.dtype), torch.float32)
        return sampling.boundary_step(noise_pred, t, s, latent, self.model.scheduler.config.prediction_type, alpha_schedule,
                                      sigma_schedule, out_dtype, self._consts)

    @torch.no_grad()
    def cons_generation(self, latent, guidance_scale=1, dynamic_guidance=False, tau1=0.4, tau2=0.6, w_embed_dim=0,
                        controller=None):
        """Reverse (noise -> data) consistency sampling: one UNet call + one boundary step per (t, s) pair."""
        all_latent = [latent]
        latent = latent.clone().detach()
        alpha_schedule, sigma_schedule = sampling.schedules(self.model.scheduler)
        # dynamic guidance is the reference's editing schedule (utils/generation.py:74-82): such passes run at the accurate precision
        # level of the native UNet, like the inversion loop and every pass with a controller attached (unet.py: precision policy)
        with sampling.editing(self.reverse_cons_model, dynamic_guidance):
            for t, s in zip(self.reverse_timesteps, self.reverse_boundary_timesteps):
                noise_pred = self.get_noise_pred(model=self.reverse_cons_model, latent=latent, t=t, context=None, tau1=tau1,
                                                 tau2=tau2, w_embed_dim=w_embed_dim, guidance_scale=guidance_scale,
                                                 dynamic_guidance=dynamic_guidance)
                latent = self._boundary_step(noise_pred, t, s, latent, alpha_schedule, sigma_schedule)
                if controller is not None:
                    latent = controller.step_callback(latent)
                all_latent.append(latent)
        return all_latent

    @torch.no_grad()
    def cons_inversion(self, image, guidance_scale=0.0, w_embed_dim=0, seed=0, device_images=False):
        """Forward (data -> noise) consistency inversion from a noised encoding at `start_timestep`.

        device_images (uint8 images on the device): image_rec is the pair (the images at 512 x 512, the whole decoded batch), both
        uint8 NHWC on the device.

        `seed` may be a list with one seed per image (batched editing): image g is noised with
        randn((1, ...), generator=manual_seed(seed[g])) and every row is what an inversion of that image alone with seed[g] gives.
        An int keeps the one batch-wide draw."""
        alpha_schedule, sigma_schedule = sampling.schedules(self.model.scheduler)
        latent, image_gt = self.image2latent(image, return_bytes=True) if device_images else (self.image2latent(image), None)
        groups = None
        if isinstance(seed, (list, tuple)):
            if len(seed) != latent.shape[0]:
                raise ValueError(f"cons_inversion: {len(seed)} seeds for {latent.shape[0]} images")
            noise = torch.cat([torch.randn((1, *latent.shape[1:]), generator=torch.Generator().manual_seed(int(sd))) for sd in seed])
            noise = noise.to(latent.device)
            groups = (latent.shape[0], 1)
        else:
            noise = torch.randn(latent.shape, generator=torch.Generator().manual_seed(seed)).to(latent.device)
        latent = self.noise_scheduler.add_noise(latent, noise, torch.tensor([self.start_timestep]))
        image_rec = (image_gt, self.latent2image(latent, return_type='uint8_device')) if device_images else self.latent2image(latent)
        prev_groups, self.prompt_groups = self.prompt_groups, groups
        try:
            with sampling.editing(self.forward_cons_model, True):    # forward steps amplify the per-evaluation error: accurate precision level
                for t, s in zip(self.forward_timesteps, self.forward_boundary_timesteps):
                    noise_pred = self.get_noise_pred(model=self.forward_cons_model, latent=latent, t=t, context=None,
                                                     guidance_scale=guidance_scale, w_embed_dim=w_embed_dim, dynamic_guidance=False)
                    latent = self._boundary_step(noise_pred, t, s, latent, alpha_schedule, sigma_schedule)
        finally:
            self.prompt_groups = prev_groups
        return image_rec, [latent]


# ----------------------------------------------------------------------------------------------------------- misc utils
def _to_uint8_device(image):
    """decoded NCHW sample -> uint8 NHWC on its device: clamp, scale and truncate towards zero in the sample's own dtype, the values
    `(image * 255).astype(np.uint8)` takes on the host (the same elementwise arithmetic; the values lie in [0, 255])."""
    if image.is_cuda and image.dim() == 4 and image.shape[1] == 3 and image.is_contiguous() and image.dtype in (torch.float16, torch.float32):
        from . import ops
        return ops.image_to_u8(image)                  # the same bytes in one launch (icd_image_to_u8)
    image = (image / 2 + 0.5).clamp(0, 1)
    return (image.permute(0, 2, 3, 1) * 255).to(torch.uint8).contiguous()


def _to_uint8_host(image):
    """decoded NCHW sample -> uint8 NHWC numpy array, the reference's conversion (utils/generation.py)"""
    image = (image / 2 + 0.5).clamp(0, 1)
    image = image.cpu().permute(0, 2, 3, 1).numpy()
    return (image * 255).astype(np.uint8)


def _is_device_images(image):
    """uint8 NHWC images on the device: a [B, H, W, 3] tensor or a list of [H, W, 3] tensors"""
    if type(image) is torch.Tensor:
        return image.dtype == torch.uint8 and image.is_cuda and image.dim() == 4
    return type(image) is list and len(image) > 0 and all(
        type(i) is torch.Tensor and i.dtype == torch.uint8 and i.is_cuda and i.dim() == 3 for i in image)


def latent2image(vae, latents, on_device=False):
    """uint8 NHWC images: a numpy array, or with on_device=True a tensor that stays on the device."""
    image = vae.decode(1 / 0.18215 * latents)['sample']
    return _to_uint8_device(image) if on_device else _to_uint8_host(image)


def init_latent(latent, model, height, width, generator, batch_size):
    """ONE noise sample, expanded to the batch (utils/generation.py:536-543)."""
    if latent is None:
        latent = torch.randn((1, model.unet.in_channels, height // 8, width // 8), generator=generator)
    latents = latent.expand(batch_size, model.unet.in_channels, height // 8, width // 8).to(model.device)
    return latent, latents


def init_latent_groups(latent, model, height, width, generator, n_groups, n_prompts):
    """init_latent per prompt group: G noise samples (one call of the generator when `latent` is None), each repeated for the P
    prompts of its group -> ([G, 4, h, w], [G * P, 4, h, w] group-major)."""
    shape = (model.unet.in_channels, height // 8, width // 8)
    if latent is None:
        latent = torch.randn((n_groups, *shape), generator=generator)
    if tuple(latent.shape) != (n_groups, *shape):
        raise ValueError(f"runner: latent of shape {tuple(latent.shape)} for {n_groups} prompt groups (expected {(n_groups, *shape)})")
    latents = latent[:, None].expand(n_groups, n_prompts, *shape).reshape(n_groups * n_prompts, *shape).to(model.device)
    return latent, latents


def load_512(image_path, left=0, right=0, top=0, bottom=0, device=None):
    """device=None: the reference's function, the file resized to 512 x 512 on the host.  With a device the file's RGB bytes are
    uploaded as they are, uint8 [H, W, 3]; Generator.image2latent resizes them there (the same bytes, icd_vae_ingest)."""
    from PIL import Image
    image = np.array(Image.open(image_path).convert('RGB'))[:, :, :3]
    if device is not None:
        return torch.from_numpy(np.ascontiguousarray(image)).to(device)
    return np.array(Image.fromarray(image).resize((512, 512)))


def to_pil_images(images, num_rows=1, offset_ratio=0.02):
    from PIL import Image
    if type(images) is list:
        num_empty = len(images) % num_rows
    elif images.ndim == 4:
        num_empty = images.shape[0] % num_rows
    else:
        images, num_empty = [images], 0
    blank = np.ones(images[0].shape, dtype=np.uint8) * 255
    tiles = [im.astype(np.uint8) for im in images] + [blank] * num_empty
    h, w, _ = tiles[0].shape
    gap = int(h * offset_ratio)
    cols = len(tiles) // num_rows
    canvas = np.ones((h * num_rows + gap * (num_rows - 1), w * cols + gap * (cols - 1), 3), dtype=np.uint8) * 255
    for r in range(num_rows):
        for c in range(cols):
            canvas[r * (h + gap): r * (h + gap) + h, c * (w + gap): c * (w + gap) + w] = tiles[r * cols + c]
    return Image.fromarray(canvas)


def view_images(images, num_rows=1, offset_ratio=0.02):
    img = to_pil_images(images, num_rows, offset_ratio)
    try:
        from IPython.display import display
        display(img)
    except ImportError:
        pass
    return img
