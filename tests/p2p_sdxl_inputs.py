"""Inputs shared by the SDXL prompt-to-prompt tests (CPU and GPU): cross-attention maps with a spatial blob on a few word columns, so that
LocalBlend's normalised heat has structure on both sides of its threshold, and the torch expression of LocalBlend.__call__."""
import torch
import torch.nn.functional as F

N_WORDS = 77
MAIN_WORDS, SUB_WORDS = (2, 5), (7,)


def blend_inputs(seed, P, heads, n_layers, res, latent, x_dtype=torch.float16, layer_heads=None, channels=4, n_words=N_WORDS):
    """(maps: n_layers fp16 CPU tensors [P * heads, res * res, 77], alpha [P, 77], alpha_sub [P, 77], x [P, 4, latent, latent]).
    layer_heads: a list of head counts, one per layer (then `heads` and `n_layers` are not read); latent: a side or (H, W); channels and
    n_words: of x and of the maps.  The defaults draw what they always drew."""
    gen = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(res).float(), torch.arange(res).float(), indexing="ij")
    s = res / 16.0
    centres = {2: (4.0, 5.0), 5: (11.0, 9.0), 7: (8.0, 3.0)}
    maps = []
    for li, h in enumerate([heads] * n_layers if layer_heads is None else layer_heads):
        m = torch.rand(P * h, res * res, n_words, generator=gen) * 0.02
        for w, (cy, cx) in centres.items():
            blob = torch.exp(-((yy - s * cy - 0.05 * s * li) ** 2 + (xx - s * cx) ** 2) / (8.0 * s * s)).reshape(1, res * res)
            m[:, :, w] = m[:, :, w] * 10.0 * (0.05 + blob) * (1 + 0.1 * torch.rand(P * h, 1, generator=gen))
        maps.append(m.half())
    alpha = torch.zeros(P, n_words)
    alpha[:, list(MAIN_WORDS)] = 1
    sub = torch.zeros(P, n_words)
    sub[:, list(SUB_WORDS)] = 1
    H, W = (latent, latent) if isinstance(latent, int) else latent
    x = torch.randn(P, channels, H, W, generator=gen).to(x_dtype)
    return maps, alpha, sub, x


def blend_masks(maps, alpha, sub, th, size, dtype):
    """The masks of LocalBlend.get_mask (utils/p2p.py:20-31) evaluated in `dtype` on the fp16 maps, layer by layer so that a
    50-layer store never exists twice: (main-word mask, mask with the substruct words cleared), bool [P, 1, H, W]."""
    P = alpha.shape[0]
    res = int(round(maps[0].shape[1] ** 0.5))
    out = []
    for al, pool in ((alpha, True), (sub, False)):
        al = al.to(maps[0].device, dtype).reshape(P, 1, 1, 1, 1, N_WORDS)
        cols = torch.nonzero(al.reshape(P, N_WORDS).sum(0)).flatten()
        # (maps * alpha).sum(-1).mean(1): the words that alpha leaves out contribute exact zeros, so only its columns are read
        heat = torch.cat([(m.reshape(P, -1, 1, res, res, N_WORDS)[..., cols].to(dtype) * al[..., cols]).sum(-1) for m in maps], dim=1).mean(1)
        heat = heat.float() if dtype == torch.float16 and not heat.is_cuda else heat      # (CPU max_pool2d has no fp16 kernel; values unchanged)
        if pool:
            heat = F.max_pool2d(heat, kernel_size=3, stride=1, padding=1)
        heat = F.interpolate(heat, size=size)
        heat = heat / heat.amax(dim=(2, 3), keepdim=True)
        on = heat.gt(th)
        out.append(on[:1] + on)
    return out[0], out[0] * ~out[1]


def blend_with(mask, x):
    return x[:1] + mask.float() * (x - x[:1])
