#!/usr/bin/env python3
"""Editing with the quality metrics on the device: G [source, edit] pairs edited in one U-Net batch, decoded and scored without a host copy.

    python tools/edit_metrics_bench.py [--pairs 8] [--reps 3] [--no-host-route] [--dinov2] [--lpips]

Workload: tools/edit_batch_bench.py's (full-size SD1.5 on synthetic weights, 4-step consistency inversion + 4-step reverse edit with the
shipped editing settings, p2p.ControllerBatch), followed by the AutoencoderKL decode to uint8 images on the device
(generation.latent2image(..., on_device=True)) and the three scores of the reference's editing driver: preservation CLIP score (edited vs
source image), editing CLIP score (edited image vs edit prompt), PSNR (metrics.py; CLIP ViT-L/14 on seeded weights).  Prints edited
images/s, edited + scored images/s and the mean scores.  For scale it also times the route this replaces: images copied to the host,
transformers' PIL image processor, the transformers CLIP model in fp16 on the GPU.  Device windows are event-timed with a warm-up; the
host route is wall time around a synchronise (its work is on the host).  --dinov2 adds the driver's fourth device-side score,
preservation_dinov2 (metrics.calc_dinov2_images_images, dinov2-base on seeded weights), to the scored set and times it on its own as well; --lpips does the same for preservation_lpips (metrics.calculate_lpips, the VGG16 stack at
full width on seeded weights).
"""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=8)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--no-host-route", action="store_true")
ap.add_argument("--dinov2", action="store_true", help="also score preservation_dinov2 (dinov2-base on seeded weights)")
ap.add_argument("--lpips", action="store_true", help="also score preservation_lpips (VGG16 LPIPS on seeded weights)")
a = ap.parse_args()

from invertible_cd_amd import build, clip, dinov2, generation, lpips, metrics, p2p, synthetic, unet, vae
from invertible_cd_amd.pipelines import StableDiffusionPipeline
from invertible_cd_amd.schedulers import DDIMScheduler
from invertible_cd_amd.unet_config import SD15

dev, G, P = "cuda", a.pairs, 2
p2p.tokenizer, p2p.NUM_DDIM_STEPS, p2p.device = synthetic.SyntheticTokenizer(), 4, dev
PAIR = ["a cat sitting on a bench", "a dog sitting on a bench"]
net = unet.UNet2DConditionModel(SD15, synthetic.synthetic_state_dict(SD15, seed=0, device=dev, dtype=torch.float16))
kl = vae.AutoencoderKL(vae.SD_VAE, synthetic.synthetic_vae_state_dict(vae.SD_VAE, seed=0, device=dev, dtype=torch.float16), device=dev,
                       dtype=torch.float16)
model = StableDiffusionPipeline(net, DDIMScheduler.sd15(), kl, synthetic.SyntheticTokenizer(), device=dev, dtype=torch.float16)
solver = generation.Generator(model, 50, DDIMScheduler.sd15(), forward_cons_model=model, reverse_cons_model=model,
                              reverse_timesteps=[259, 519, 779, 999], forward_timesteps=[19, 259, 519, 779])
clip_sd = synthetic.synthetic_clip_state_dict(clip.CLIP_VIT_L, True, seed=0)
clip_sd.update(synthetic.synthetic_clip_vision_state_dict(clip.CLIP_VIT_L_VISION, seed=0))
scorer = clip.CLIPModel(clip.CLIP_VIT_L, clip.CLIP_VIT_L_VISION, clip_sd)
dino = dinov2.Dinov2Model(dinov2.DINOV2_BASE, synthetic.synthetic_dinov2_state_dict(dinov2.DINOV2_BASE, seed=0)) if a.dinov2 else None
lp = lpips.Lpips(lpips.LPIPS_VGG16, *synthetic.synthetic_lpips_state(lpips.LPIPS_VGG16, seed=0)) if a.lpips else None
g = torch.Generator().manual_seed(453645634 + G)
img = torch.randn(G, 4, 64, 64, generator=g).to(dev)
ctx_inv = torch.randn(2 * G, 77, 768, generator=g).to(dev, torch.float16)
ctx_edit = torch.randn(2 * G * P, 77, 768, generator=g).to(dev, torch.float16)
ids = torch.randint(3, 49405, (G, 77), generator=g)
ids[:, 0], ids[:, 20:] = 49406, 49407


def edit():
    """inversion + batched edit + decode -> uint8 [G * P, 512, 512, 3] on the device (group-major: source, edited, source, ...)."""
    solver.context = ctx_inv
    inv = solver.cons_inversion(img, guidance_scale=0.0, w_embed_dim=512, seed=list(range(G)))[1][0]
    ctrl = p2p.ControllerBatch([p2p.make_controller(PAIR, True, 0.3, 0.6, blend_words=(("cat",), ("dog",)),
                                                    equilizer_params={"words": ("dog",), "values": (4.0,)}) for _ in range(G)])
    p2p.register_attention_control(model, ctrl)
    solver.context = ctx_edit
    solver.prompt_groups = (G, P)
    try:
        lat = solver.cons_generation(inv[:, None].expand(G, P, *inv.shape[1:]).reshape(G * P, *inv.shape[1:]), guidance_scale=19.0,
                                     w_embed_dim=512, dynamic_guidance=True, tau1=0.8, tau2=0.8, controller=ctrl)[-1]
    finally:
        solver.prompt_groups = None
        p2p.register_attention_control(model, None)
    return generation.latent2image(kl, lat.to(kl.dtype), on_device=True)


def score(images):
    src, out = images[0::P].contiguous(), images[1::P].contiguous()
    assert src.is_cuda and out.is_cuda
    res = (metrics.calc_clip_score_images_images(src, out, dev, model=scorer), metrics.calc_clip_score_images_prompts(out, ids, dev, model=scorer),
           metrics.calculate_psnr(src, out, dev))
    if a.dinov2:
        res += (metrics.calc_dinov2_images_images(src, out, dev, model=dino),)
    if a.lpips:
        res += (metrics.calculate_lpips(src, out, dev, model=lp),)
    return res


def timed(fn, reps):
    r = fn()                                                         # warm-up
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        r = fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps, r


print(f"# tools/edit_metrics_bench.py on {torch.cuda.get_device_name(0)}, kernels_sha {build.source_sha()}, G = {G}, reps {a.reps}")
t_edit, images = timed(edit, a.reps)
t_both, scores = timed(lambda: score(edit()), a.reps)
t_score, _ = timed(lambda: score(images), a.reps)
pres, edsc, psnr = scores[:3]
n_scores = ("three", "four", "five")[int(a.dinov2) + int(a.lpips)]
print(f"edit (inversion + edit + decode)            {t_edit:9.1f} ms  {G / t_edit * 1e3:7.2f} edited images/s")
print(f"edit + scores on the device                 {t_both:9.1f} ms  {G / t_both * 1e3:7.2f} edited + scored images/s "
      f"({t_both / t_edit:.3f} x the edit alone)")
print(f"the {n_scores} scores alone ({2 * G} CLIP image + {G} text embeddings, {G} PSNR" + (f", {2 * G} DINOv2 embeddings" if a.dinov2 else "")
      + (f", {G} LPIPS pairs" if a.lpips else "") + f")  {t_score:9.1f} ms")
if a.dinov2:
    t_dino, _ = timed(lambda: metrics.calc_dinov2_images_images(images[0::P].contiguous(), images[1::P].contiguous(), dev, model=dino), a.reps)
    print(f"preservation_dinov2 alone ({2 * G} images: preprocessing at 256 / 224, dinov2-base, cosine)  {t_dino:9.1f} ms")
if a.lpips:
    t_lp, _ = timed(lambda: metrics.calculate_lpips(images[0::P].contiguous(), images[1::P].contiguous(), dev, model=lp), a.reps)
    print(f"preservation_lpips alone ({G} pairs: ingest at 224, VGG16 on {2 * G} images, five distance taps)  {t_lp:9.1f} ms")
mean = lambda v: float(torch.as_tensor(v, dtype=torch.float64).mean())
print(f"mean scores (synthetic weights: plumbing, not quality): preservation_clip_score {mean(pres):.4f}  editing_clip_score {mean(edsc):.4f}  "
      f"psnr {mean(psnr) if isinstance(psnr, list) else psnr:.3f} dB" + (f"  preservation_dinov2 {mean(scores[3]):.4f}" if a.dinov2 else "")
      + (f"  preservation_lpips {mean(scores[-1]):.4f}" if a.lpips else ""))

if not a.no_host_route:
    import transformers
    from PIL import Image
    tm = transformers.CLIPModel(transformers.CLIPConfig(text_config=dict(clip.CLIP_VIT_L.to_dict()), vision_config=dict(clip.CLIP_VIT_L_VISION.to_dict()),
                                                        projection_dim=768))
    own = tm.state_dict()
    tm.load_state_dict({k: clip_sd.get(k, v) for k, v in own.items()})
    tm = tm.half().to(dev).eval()
    proc = transformers.CLIPImageProcessorPil()

    @torch.no_grad()
    def host_route():
        arr = images.cpu().numpy()                                   # the device -> host copy the device route does without
        pv = proc(images=[Image.fromarray(x) for x in arr], return_tensors="pt")["pixel_values"].to(dev, torch.float16)
        ei = tm.get_image_features(pixel_values=pv)
        ei = getattr(ei, "pooler_output", ei)
        et = tm.get_text_features(input_ids=ids.to(dev))
        et = getattr(et, "pooler_output", et)
        ei, et = ei / ei.norm(dim=-1, keepdim=True), et / et.norm(dim=-1, keepdim=True)
        return (ei[0::P] * ei[1::P]).sum(-1).cpu(), (et * ei[1::P]).sum(-1).cpu(), metrics.calculate_psnr(list(arr[0::P]), list(arr[1::P]), "cpu")
    host_route()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.reps):
        h = host_route()
    torch.cuda.synchronize()
    t_host = (time.perf_counter() - t0) / a.reps * 1e3
    print(f"host route (copy to host, PIL preprocessing, transformers CLIP fp16 on the GPU, numpy PSNR)  {t_host:9.1f} ms wall  "
          f"-> {G / (t_edit + t_host) * 1e3:7.2f} edited + scored images/s;  max |score difference| to the device route: "
          f"preservation {float((h[0] - pres).abs().max()):.2e}, editing {float((h[1] - edsc).abs().max()):.2e}")
