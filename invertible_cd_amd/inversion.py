"""Image inversion entry point (API mirror of the reference's utils/inversion.py).

`invert(...)` keeps the reference signature and return value ((image_gt, image_rec), latent, uncond_embeddings).
The consistency branch (`is_cons_inversion=True` -> Generator.cons_inversion) is the hot path and runs on the native
UNet.  The DDIM-inversion branch is kept (it reuses the same UNet).  Null-text optimisation (`do_nti=True`,
utils/inversion.py:11-48) needs autograd THROUGH the UNet, which the inference-only MI355X executor does not provide:
it raises NotImplementedError (out of scope, baseline only).

Batched editing: G image paths with G prompts invert in one batch ([G, 4, 64, 64]; do_npi: per-step cond embeddings [G, 77, 768]).
With `seed` a list of G seeds, row g is exactly what `invert` of image g alone with seed=seed[g] returns; an int seed keeps the
one batch-wide noise draw.

`device_images=True` keeps the images on the device: the files' bytes are uploaded at their own sizes (load_512(..., device=)), resized
to 512 x 512 and encoded there, and image_gt / image_rec come back as uint8 NHWC device tensors ([G, 512, 512, 3], the whole batch) that
hold the bytes of the host route's arrays.
"""
from .generation import load_512
from .p2p import register_attention_control


def null_optimization(solver, latents, guidance_scale, num_inner_steps, epsilon):
    raise NotImplementedError("null-text optimisation needs autograd through the UNet; the MI355X-native path is "
                              "inference-only (use is_cons_inversion=True, the iCD forward model)")


def invert(solver, stop_step, is_cons_inversion=False, inv_guidance_scale=1, nti_guidance_scale=8, dynamic_guidance=False,
           tau1=0.4, tau2=0.6, w_embed_dim=0, image_path=None, prompt='', offsets=(0, 0, 0, 0), do_nti=False, do_npi=False,
           num_inner_steps=10, early_stop_epsilon=1e-5, seed=0, device_images=False):
    solver.init_prompt(prompt)
    uncond_embeddings, cond_embeddings = solver.context.chunk(2)
    register_attention_control(solver.model, None)
    dev = {'device': solver.model.device} if device_images else {}
    if isinstance(image_path, list):
        image_gt = [load_512(path, *offsets, **dev) for path in image_path]
    else:
        image_gt = load_512(image_path, *offsets, **dev)
        image_gt = [image_gt] if device_images else image_gt
    kw = {'device_images': True} if device_images else {}
    if is_cons_inversion:
        image_rec, latents = solver.cons_inversion(image_gt, w_embed_dim=w_embed_dim, guidance_scale=inv_guidance_scale, seed=seed, **kw)
    else:
        image_rec, latents = solver.ddim_inversion(image_gt, n_steps=stop_step, guidance_scale=inv_guidance_scale,
                                                   dynamic_guidance=dynamic_guidance, tau1=tau1, tau2=tau2, w_embed_dim=w_embed_dim, **kw)
    if device_images:
        image_gt, image_rec = image_rec                # the images at 512 x 512 and the decoded batch, both uint8 NHWC on the device
    if do_nti:
        print("Null-text optimization...")
        uncond_embeddings = null_optimization(solver, latents, nti_guidance_scale, num_inner_steps, early_stop_epsilon)
    elif do_npi:
        uncond_embeddings = [cond_embeddings] * solver.n_steps
    else:
        uncond_embeddings = None
    return (image_gt, image_rec), latents[-1], uncond_embeddings
