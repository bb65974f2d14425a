"""AutoencoderKL (the VAE either side of the iCD path) on the HIP kernels of this package - SURVEY.md section 8f rank 1.

Drop-in for the attributes the reference touches on `model.vae` / `pipe.vae`:
    vae.decode(z)['sample']                      utils/generation.py:258   (z already divided by 0.18215 by the caller)
    vae.decode(z, return_dict=False)[0]          utils/generation_sdxl.py:466
    vae.encode(x)['latent_dist'].mean            utils/generation.py:277,282
    vae.dtype, vae.config.scaling_factor, vae.to(dtype)

Architecture: diffusers 0.25.1 AutoencoderKL (oracle/vae_ref.py restates it and is what the GPU tests compare against).
Everything runs on the same operators as the UNet: GroupNorm(+SiLU) `icd_groupnorm`, 3x3 / 1x1 convs as implicit GEMM
`icd_gemm` (nearest-2x upsample folded into the loader; the encoder's bottom/right-only padding is ICD_GEMM_PAD_HI), the
mid-block attention (one head of 512 channels) flash style (`icd_attention_wide` at head dims 168 - 512, `icd_attention_fused` up to
160) or as QK^T -> row softmax -> PV (`icd_gemm` batched + `icd_softmax_rows`): AutoencoderKL._attention_kind, first / last convs through `icd_pack_nchw` + implicit GEMM and
`icd_conv_out_n`.  Host-side algebra done once at load, all exact in real arithmetic:
  * post_quant_conv (1x1 + bias) is folded into decoder.conv_in; its bias rides on a ones-channel of the packed latent
    so the 3x3 conv's zero padding still sees zeros outside the image;
  * quant_conv is folded into encoder.conv_out (mean rows and log-variance rows as two 4-channel output convs);
  * the V bias of the attention is folded into the output projection's bias (softmax rows sum to one).
Two arithmetic modes, selected like the reference does it, through `vae.to(dtype)`:
  * fp16 (default, `AutoencoderKL(..., dtype=torch.float16)` / `.to(torch.float16)`): activations are fp16 token-major
    [B*H*W, C] with fp32 accumulation, like the UNet.
  * fp32 fidelity (`.to(torch.float32)` - what utils/generation_sdxl.py:465-466 and diffusers' force_upcast ask for,
    because real SDXL-VAE activations overflow the fp16 range): every tensor that can grow without bound (conv outputs, the
    residual stream) is stored in fp32; the operands of the matrix cores are "split3" fp16 tensors [hi | lo | hi] against
    weights packed [w_hi | w_hi | w_lo] (ops.split_weight), i.e. (a_hi + a_lo)(w_hi + w_lo) minus the lo*lo term, ~2^-21
    relative operand error on the unchanged fp16 MFMA kernels at 3x their work; GroupNorm reads fp32 and writes split3
    (icd_groupnorm_f32_split); tensors that reach a conv without a GroupNorm (Up/Downsample, conv_shortcut) are scaled by a
    power of two chosen from their max |x| (icd_absmax) on the way to fp16 and the conv's alpha restores the scale exactly
    (icd_split_cast).  Only the
    mid-block attention keeps fp16 q / k / v / P (bounded by construction: they follow a GroupNorm and a softmax).
Layout of this file.  The topology exists once: VAEConfig.levels enumerates the blocks (for state_dict_shapes and the walks), and
AutoencoderKL._resnet / _attention / _mid / _decode_body / _encode_body walk them in an arithmetic object, _Fp16Carry or _Fp32Split,
that AutoencoderKL._arithmetic picks once per call from `dtype`.  The two differ only in what a residual stream is, the GroupNorm that
reads it, how a launch that produces a stream or reads the raw stream is issued, the weight dictionary, the pack of the first operand and
the upsampler (phase form in fp16 only).  The folds exist once too: _fold_state_dict gives fp32 masters under the kernels' keys;
pack_vae_state_dict (fp16, at load) and _split_vae_weights (split3, on the first fp32 use, from the retained state dict) map over them.
"""
from dataclasses import dataclass, replace
from types import SimpleNamespace
from typing import Tuple

import torch

from . import ops

EPS = 1e-6


@dataclass(frozen=True)
class VAEConfig:
    in_channels: int = 3
    out_channels: int = 3
    latent_channels: int = 4
    block_out_channels: Tuple[int, ...] = (128, 256, 512, 512)
    layers_per_block: int = 2
    norm_num_groups: int = 32
    scaling_factor: float = 0.18215

    def scaled(self, block_out_channels):
        """Reduced-width copy (tests): channel counts must stay multiples of 32 (GroupNorm groups) ."""
        return replace(self, block_out_channels=tuple(block_out_channels))

    def levels(self, side):
        """The resolution levels of one side, "encoder" or "decoder", in execution order: ([(resnet prefix, cin, cout), ...], prefix of
        the Down/Upsample2D conv that ends the level or None, the level's channels).  The one place that knows the block key strings."""
        enc = side == "encoder"
        ch = list(self.block_out_channels) if enc else list(self.block_out_channels)[::-1]
        blocks, resample = ("down_blocks", "downsamplers") if enc else ("up_blocks", "upsamplers")
        cin = ch[0]
        for i, c in enumerate(ch):
            resnets = []
            for j in range(self.layers_per_block + (not enc)):
                resnets.append((f"{side}.{blocks}.{i}.resnets.{j}.", cin, c))
                cin = c
            yield resnets, f"{side}.{blocks}.{i}.{resample}.0.conv." if i < len(ch) - 1 else None, c

    def state_dict_shapes(self):
        """diffusers AutoencoderKL keys -> shapes (same layout the oracle pins by the exact SD VAE parameter count)."""
        ch, zc = list(self.block_out_channels), self.latent_channels
        out = {}

        def resnet(p, cin, cout):
            out[p + "norm1.weight"] = (cin,); out[p + "norm1.bias"] = (cin,)
            out[p + "conv1.weight"] = (cout, cin, 3, 3); out[p + "conv1.bias"] = (cout,)
            out[p + "norm2.weight"] = (cout,); out[p + "norm2.bias"] = (cout,)
            out[p + "conv2.weight"] = (cout, cout, 3, 3); out[p + "conv2.bias"] = (cout,)
            if cin != cout:
                out[p + "conv_shortcut.weight"] = (cout, cin, 1, 1); out[p + "conv_shortcut.bias"] = (cout,)

        def mid(p, c):
            resnet(p + "resnets.0.", c, c)
            a = p + "attentions.0."
            out[a + "group_norm.weight"] = (c,); out[a + "group_norm.bias"] = (c,)
            for n in ("to_q", "to_k", "to_v", "to_out.0"):
                out[a + n + ".weight"] = (c, c); out[a + n + ".bias"] = (c,)
            resnet(p + "resnets.1.", c, c)

        def levels(side):
            for resnets, resample, c in self.levels(side):
                for p, cin, cout in resnets:
                    resnet(p, cin, cout)
                if resample:
                    out[resample + "weight"] = (c, c, 3, 3); out[resample + "bias"] = (c,)

        out["encoder.conv_in.weight"] = (ch[0], self.in_channels, 3, 3); out["encoder.conv_in.bias"] = (ch[0],)
        levels("encoder")
        mid("encoder.mid_block.", ch[-1])
        out["encoder.conv_norm_out.weight"] = (ch[-1],); out["encoder.conv_norm_out.bias"] = (ch[-1],)
        out["encoder.conv_out.weight"] = (2 * zc, ch[-1], 3, 3); out["encoder.conv_out.bias"] = (2 * zc,)
        out["quant_conv.weight"] = (2 * zc, 2 * zc, 1, 1); out["quant_conv.bias"] = (2 * zc,)
        out["post_quant_conv.weight"] = (zc, zc, 1, 1); out["post_quant_conv.bias"] = (zc,)
        rev = ch[::-1]
        out["decoder.conv_in.weight"] = (rev[0], zc, 3, 3); out["decoder.conv_in.bias"] = (rev[0],)
        mid("decoder.mid_block.", rev[0])
        levels("decoder")
        out["decoder.conv_norm_out.weight"] = (rev[-1],); out["decoder.conv_norm_out.bias"] = (rev[-1],)
        out["decoder.conv_out.weight"] = (self.out_channels, rev[-1], 3, 3); out["decoder.conv_out.bias"] = (self.out_channels,)
        return out


SD_VAE = VAEConfig()
SDXL_VAE = VAEConfig(scaling_factor=0.13025)


class _Out(dict):
    """dict with attribute access: the reference indexes `['sample']` / `['latent_dist']`, diffusers pipelines use `.x`."""
    __getattr__ = dict.__getitem__


class LatentDist:
    """diffusers' `DiagonalGaussianDistribution` over the 8 moment channels of quant_conv(encoder(x)).

    The SD1.5 path reads `.mean` (utils/generation.py:277,282); the SDXL img2img `prepare_latents` the reference calls at
    utils/generation_sdxl.py:273-276 draws `.sample(generator)`: mean + exp(0.5 * clamp(logvar, -30, 20)) * randn, the
    noise drawn like diffusers' randn_tensor (a CPU generator draws on the CPU in the parameters' dtype, then moves)."""

    def __init__(self, mean, logvar=None):
        self.mean = mean
        self.logvar = None if logvar is None else torch.clamp(logvar, -30.0, 20.0)
        self.deterministic = logvar is None
        if self.logvar is not None:
            self.std = torch.exp(0.5 * self.logvar)
            self.var = torch.exp(self.logvar)
        else:
            self.std = self.var = torch.zeros_like(mean)

    def mode(self):
        return self.mean

    def sample(self, generator=None):
        gen_dev = generator.device.type if generator is not None else self.mean.device.type
        if gen_dev == "cpu":
            noise = torch.randn(self.mean.shape, generator=generator, device="cpu", dtype=self.mean.dtype).to(self.mean.device)
        else:
            noise = torch.randn(self.mean.shape, generator=generator, device=self.mean.device, dtype=self.mean.dtype)
        return self.mean + self.std * noise


def _pad(t, n, dim=0):
    """t zero-padded to n along dim"""
    out = torch.zeros(*t.shape[:dim], n, *t.shape[dim + 1:])
    out.narrow(dim, 0, t.shape[dim]).copy_(t)
    return out


def _fold_state_dict(cfg: VAEConfig, sd):
    """diffusers-layout AutoencoderKL state dict -> fp32 masters on the host under the kernels' keys, the module docstring's folds applied:
    convs [O, I, kh, kw] (the first convs padded to 8 input channels, the last ones to 4 outputs), projections [O, I], biases / affine."""
    f32 = lambda k: sd[k].detach().to("cpu", torch.float32)
    zc = cfg.latent_channels
    folded = ("quant_conv.", "post_quant_conv.", "encoder.conv_out.", "decoder.conv_out.")
    M = {k: f32(k) for k in cfg.state_dict_shapes() if not k.startswith(folded) and ".attentions.0.to_" not in k}
    for a in ("encoder.mid_block.attentions.0.", "decoder.mid_block.attentions.0."):
        M[a + "to_qk.weight"] = torch.cat([f32(a + "to_q.weight"), f32(a + "to_k.weight")])
        M[a + "to_qk.bias"] = torch.cat([f32(a + "to_q.bias"), f32(a + "to_k.bias")])
        M[a + "to_v.weight"] = f32(a + "to_v.weight")
        wo = M[a + "to_out.weight"] = f32(a + "to_out.0.weight")
        M[a + "to_out.bias"] = wo @ f32(a + "to_v.bias") + f32(a + "to_out.0.bias")             # softmax rows sum to one
    M["encoder.conv_in.weight"] = _pad(M["encoder.conv_in.weight"], 8, dim=1)
    wq, bq = f32("quant_conv.weight").reshape(2 * zc, 2 * zc), f32("quant_conv.bias")
    wo, bo = f32("encoder.conv_out.weight"), f32("encoder.conv_out.bias")
    for name, r in (("mean", slice(0, zc)), ("logvar", slice(zc, None))):    # rows of quant_conv(conv_out(.)): latent_dist.mean / .std
        M[f"encoder.conv_out_{name}.weight"] = _pad(torch.einsum("om,mchw->ochw", wq[r], wo), 4)
        M[f"encoder.conv_out_{name}.bias"] = _pad(wq[r] @ bo + bq[r], 4)
    wpq, bpq = f32("post_quant_conv.weight").reshape(zc, zc), f32("post_quant_conv.bias")
    wi = M["decoder.conv_in.weight"]
    w8 = torch.zeros(wi.shape[0], 8, 3, 3)
    w8[:, :zc] = torch.einsum("ochw,cd->odhw", wi, wpq)
    w8[:, zc] = torch.einsum("ochw,c->ohw", wi, bpq)                          # rides on the ones channel
    M["decoder.conv_in.weight"] = w8
    M["decoder.conv_out.weight"], M["decoder.conv_out.bias"] = _pad(f32("decoder.conv_out.weight"), 4), _pad(f32("decoder.conv_out.bias"), 4)
    return M


def pack_vae_state_dict(cfg: VAEConfig, sd, device="cuda"):
    """diffusers-layout AutoencoderKL state dict -> kernel layout (fp16 weights, fp32 biases / affine)."""
    missing = [k for k in cfg.state_dict_shapes() if k not in sd]
    if missing:
        raise KeyError(f"AutoencoderKL state dict lacks {len(missing)} tensors, e.g. {missing[:3]}")
    for k, shp in cfg.state_dict_shapes().items():
        if tuple(sd[k].shape) != tuple(shp):
            raise ValueError(f"{k}: expected shape {tuple(shp)}, got {tuple(sd[k].shape)}")
    from .unet import upsample_phase_weights
    P = {}
    for k, t in _fold_state_dict(cfg, sd).items():
        if t.dim() == 1:                                                      # a bias or a GroupNorm's affine
            P[k] = t.to(device=device, dtype=torch.float32).contiguous()
            continue
        P[k] = (ops.pack_conv_weight(t) if t.dim() == 4 else t).to(device=device, dtype=torch.float16).contiguous()
        if ".upsamplers." in k:
            # the phase form of Upsample2D (four 2 x 2 convs on the input grid with tap-summed weights: 4/9 of the flops, unet.py)
            for ph, wp in enumerate(upsample_phase_weights(t)):
                P[k[:-len("weight")] + f"phase.{ph}"] = wp.reshape(wp.shape[0], -1).to(device=device, dtype=torch.float16).contiguous()
    return P


def _split_vae_weights(M, device):
    """[w_hi | w_hi | w_lo] per tap, from the fp32 masters, for every conv / projection whose input is a split3 tensor"""
    S = {}
    for k, t in M.items():
        if t.dim() == 4:
            S[k] = ops.split_weight(t.permute(0, 2, 3, 1)).reshape(t.shape[0], -1).to(device)          # [O, taps * 3I]
        elif k.endswith(("to_qk.weight", "to_v.weight")):
            S[k] = ops.split_weight(t).to(device)
    return S


def _pack32(x_nchw, device, ones_channel=-1):
    """NCHW fp32 (<= 8 channels) -> split3 [B*H*W, 24] of the 8-channel token-major packing (data movement + split only)."""
    B, Cc, H, W = x_nchw.shape
    t = torch.zeros((B, H, W, 8), device=device, dtype=torch.float32)
    t[..., :Cc] = x_nchw.to(device, torch.float32).permute(0, 2, 3, 1)
    if ones_channel >= 0:
        t[..., ones_channel] = 1.0
    return ops.split_cast(t.reshape(B * H * W, 8), 1.0)


# The two arithmetics the one topology walk of AutoencoderKL runs in.  Each says what a residual stream is and supplies: `w` / `ws` (biases,
# affine and the plain fp16 weights / the weights its operands multiply), pack (the first operand), norm (a GroupNorm of the stream -> an
# operand), issue (a conv or GEMM whose result is a stream, with an optional stream as residual), raw (the stream itself as an operand, with
# the launch arguments that undo what that took) and upsample.  `rows` is the row count of issue's result.
class _Fp16Carry:
    """A stream is the pair (x, xc): fp16 token-major x and the rounding error of its last x <- x + f(x) in one bf8 byte per element
    (icd_gemm_desc.resid_carry / out_carry, the UNet's residual mode 2); every GroupNorm normalises fp16 + carry (icd_groupnorm_carry), so
    the stream behaves like a 14-bit-mantissa tensor.  xc None (always, with carry=False): the plain fp16 stream."""
    out_dtype = torch.float16

    def __init__(self, w, groups, carry, upsample_phases):
        self.w = self.ws = w
        self.groups, self.carry, self.upsample_phases = groups, carry, upsample_phases

    def pack(self, x_nchw, ones_channel=-1):
        return ops.pack_nchw(x_nchw, ones_channel=ones_channel)

    def norm(self, s, B, HW, k, silu):
        (x, xc), w = s, self.w
        if xc is None:
            return ops.groupnorm(x, B, HW, w[k + "weight"], w[k + "bias"], EPS, silu, groups=self.groups)
        return ops.groupnorm_carry(x, B, HW, w[k + "weight"], w[k + "bias"], EPS, silu, carry=xc, groups=self.groups)

    def _oc(self, rows, cols, like):
        return torch.empty((rows, cols), device=like.device, dtype=torch.uint8) if self.carry else None

    def issue(self, fn, a, geom, weight, bias, rows, resid=(None, None), **kw):
        oc = self._oc(rows, weight.shape[0], a)
        return fn(a, *geom, weight, bias, resid=resid[0], resid_carry=resid[1], out_carry=oc, **kw), oc

    def raw(self, s):
        return s[0], {}

    def upsample(self, s, B, H, W, k):
        """Upsample2D as four 2 x 2 convs on the input grid (4/9 of its flops); upsample_phases=False, or a map one pixel wide: 3 x 3 form"""
        x, w = s[0], self.w
        if not (self.upsample_phases and W >= 2):
            return self.issue(ops.conv3x3, x, (B, H, W), w[k + "weight"], w[k + "bias"], B * 4 * H * W, upsample=True)
        uc = self._oc(B * 4 * H * W, x.shape[-1], x)
        up = torch.empty((B * 4 * H * W, x.shape[-1]), device=x.device, dtype=torch.float16)
        for ph in range(4):
            ops.conv3x3(x, B, H, W, w[k + f"phase.{ph}"], w[k + "bias"], phase=ph, out=up, out_carry=uc)
        return up, uc


class _Fp32Split:
    """A stream is one fp32 tensor; operands are split3 fp16 [hi | lo | hi] against `ws`, weights packed [w_hi | w_hi | w_lo]."""
    out_dtype = torch.float32

    def __init__(self, w, ws, groups, device):
        self.w, self.ws, self.groups, self.device = w, ws, groups, device

    def pack(self, x_nchw, ones_channel=-1):
        return _pack32(x_nchw, self.device, ones_channel)

    def norm(self, s, B, HW, k, silu):
        return ops.groupnorm_f32_split(s, B, HW, self.w[k + "weight"], self.w[k + "bias"], EPS, silu, groups=self.groups)

    def issue(self, fn, a, geom, weight, bias, rows, resid=None, **kw):
        return fn(a, *geom, weight, bias, resid=resid, out_f32=True, **kw)

    def raw(self, s):
        xs, inv = ops.split_cast_guarded(s)
        return xs, {"alpha": inv}

    def upsample(self, s, B, H, W, k):
        xs, kw = self.raw(s)
        return self.issue(ops.conv3x3, xs, (B, H, W), self.ws[k + "weight"], self.w[k + "bias"], B * 4 * H * W, upsample=True, **kw)


class AutoencoderKL:
    def __init__(self, cfg: VAEConfig, state_dict, device="cuda", dtype=torch.float16, max_chunk=8, fused_attention=None):
        if cfg.latent_channels != 4 or cfg.in_channels > 4 or cfg.out_channels > 4:
            raise ValueError("AutoencoderKL: this build supports 4 latent channels and <= 4 image channels")
        if any(c % 32 for c in cfg.block_out_channels):
            raise ValueError("AutoencoderKL: block_out_channels must be multiples of 32")
        self.cfg, self.device, self.dtype = cfg, torch.device(device), dtype
        self.config = SimpleNamespace(scaling_factor=cfg.scaling_factor, latent_channels=cfg.latent_channels,
                                      block_out_channels=list(cfg.block_out_channels), in_channels=cfg.in_channels,
                                      out_channels=cfg.out_channels)
        self.w = pack_vae_state_dict(cfg, state_dict, device)
        self._sd_ref = {k: state_dict[k] for k in cfg.state_dict_shapes()}     # masters of the fp32-fidelity weights (converted lazily)
        self._ws = None                        # split3 weights of the fp32-fidelity path, packed on first use
        self.max_chunk = max_chunk            # samples per pass (bounds the 512x512x128-channel activations and the scores)
        self.fused_attention = fused_attention    # None: _attention_kind's default; True: flash wherever a kernel has the head dim (<= 512); False: materialised scores
        self.carry = True                         # fp16 path: error-carried residual stream + GroupNorm over fp16 + carry (round 6); False: plain fp16 stream
        self.upsample_phases = True               # fp16 decoder: Upsample2D as four 2 x 2 convs on the input grid (4/9 of its flops); False: 3 x 3 form

    # -- diffusers plumbing the reference uses
    def to(self, *args, **kw):
        for a in list(args) + [kw.get("dtype")]:
            if isinstance(a, torch.dtype):
                self.dtype = a                 # float32 selects the fp32-fidelity arithmetic (module docstring), not just the I/O dtype
        return self

    # ------------------------------------------------------------------ the mid-block attention of both paths (one head of C channels)
    def _attention_kind(self, B, N, C, ld):
        """"fused" (icd_attention_fused, C <= 160), "wide" (icd_attention_wide, 160 < C <= 512) or "scores" (three launches around a
        materialised [B, N, ld] fp32 score tensor, chunked over the batch to <= 1 GiB of it)."""
        flash = "fused" if C <= 160 else "wide" if C <= 512 else "scores"
        if self.fused_attention is not None:
            return flash if self.fused_attention else "scores"
        if flash != "wide":
            return flash
        # The default at 160 < C <= 512: the wide kernel only where ONE sample's scores exceed the 1 GiB step of the materialised path
        # (more than 16384 tokens: images above 1024^2, which that path cannot hold to its step at all).  Below that the wide kernel
        # was measured slower at every size (profiles/attn_wide.txt, attention alone at d = 512, wide / materialised ms):
        #     B = 8 N = 1024   0.076 / 0.050      B = 8 N = 4096   1.085 / 0.608      B = 2 N = 16384   4.224 / 3.552
        # and decode with it 2 - 3 % slower per image (512^2 B = 8: 3.44 / 3.37 ms, 1024^2 B = 2: 16.18 / 15.74 ms), so the default
        # keeps the materialised path there; fused_attention=True selects the wide kernel at any size (no N^2 memory).
        return "wide" if N * ld * 4 > 1 << 30 else "scores"

    def _attend(self, q, k, vt, B, N, C, ld, scale):
        kind = self._attention_kind(B, N, C, ld)
        if kind == "fused":
            return ops.attention_fused(q, k, vt, B, 1, N, N, C, scale)
        if kind == "wide":
            return ops.attention_wide(q, k, vt, B, 1, N, N, C, scale)
        o = torch.empty((B * N, C), device=q.device, dtype=torch.float16)
        step = max(1, min(B, (1 << 30) // (N * ld * 4)))                        # <= 1 GiB of fp32 scores at a time
        for b0 in range(0, B, step):
            bc = min(step, B - b0)
            s = ops.attention_scores(q[b0 * N:(b0 + bc) * N], k[b0 * N:(b0 + bc) * N], bc, 1, N, N, C, scale, ld)
            pr = ops.softmax_rows(s.reshape(bc * N, ld), N, ld).reshape(bc, N, ld)
            ops.attention_apply(pr, vt[b0:b0 + bc], bc, 1, N, C, out=o[b0 * N:(b0 + bc) * N])
        return o

    def eval(self):
        return self

    # ------------------------------------------------------------------ the topology, once, in the arithmetic `A` that _arithmetic picked
    def _arithmetic(self):
        if self.dtype != torch.float32:
            return _Fp16Carry(self.w, self.cfg.norm_num_groups, self.carry, self.upsample_phases)
        if self._ws is None:
            self._ws = _split_vae_weights(_fold_state_dict(self.cfg, self._sd_ref), self.device)
        return _Fp32Split(self.w, self._ws, self.cfg.norm_num_groups, self.device)

    def _resnet(self, A, p, s, B, H, W):
        w, ws, n = A.w, A.ws, B * H * W
        h = A.norm(s, B, H * W, p + "norm1.", True)
        h = A.issue(ops.conv3x3, h, (B, H, W), ws[p + "conv1.weight"], w[p + "conv1.bias"], n)
        h = A.norm(h, B, H * W, p + "norm2.", True)
        sc = s
        if p + "conv_shortcut.weight" in ws:
            x, undo = A.raw(s)
            sc = A.issue(ops.gemm, x, (), ws[p + "conv_shortcut.weight"], w[p + "conv_shortcut.bias"], n, **undo)
        return A.issue(ops.conv3x3, h, (B, H, W), ws[p + "conv2.weight"], w[p + "conv2.bias"], n, resid=sc)

    def _attention(self, A, p, s, B, H, W):
        """q / k / v / P stay fp16 in both arithmetics (bounded by construction: they follow a GroupNorm and a softmax)"""
        w, ws = A.w, A.ws
        C, N = w[p + "to_out.weight"].shape[0], H * W
        h = A.norm(s, B, N, p + "group_norm.", False)
        qk = ops.gemm(h, ws[p + "to_qk.weight"], w[p + "to_qk.bias"])
        q, k = qk[:, :C], qk[:, C:]
        ld = (N + 7) // 8 * 8
        vt = ops.project_vt(h, ws[p + "to_v.weight"], B, N, ld)
        scale = C ** -0.5
        o = self._attend(q, k, vt, B, N, C, ld, scale)
        return A.issue(ops.gemm, o, (), w[p + "to_out.weight"], w[p + "to_out.bias"], B * N, resid=s)

    def _mid(self, A, p, s, B, H, W):
        s = self._resnet(A, p + "resnets.0.", s, B, H, W)
        s = self._attention(A, p + "attentions.0.", s, B, H, W)
        return self._resnet(A, p + "resnets.1.", s, B, H, W)

    def _decode_body(self, A, x, B, H, W):
        """x: conv_in's operand, the packed latent with its ones channel (A.pack) -> image [B, 3, 8H, 8W] in A.out_dtype"""
        w, ws, cfg = A.w, A.ws, self.cfg
        s = A.issue(ops.conv3x3, x, (B, H, W), ws["decoder.conv_in.weight"], w["decoder.conv_in.bias"], B * H * W)
        s = self._mid(A, "decoder.mid_block.", s, B, H, W)
        for resnets, up, _ in cfg.levels("decoder"):
            for p, _, _ in resnets:
                s = self._resnet(A, p, s, B, H, W)
            if up:
                s = A.upsample(s, B, H, W, up)
                H, W = 2 * H, 2 * W
        h = A.norm(s, B, H * W, "decoder.conv_norm_out.", True)
        return ops.conv_out(h, B, H, W, ws["decoder.conv_out.weight"], w["decoder.conv_out.bias"], out_dtype=A.out_dtype, cout=cfg.out_channels)

    def _encode_body(self, A, x, B, H, W):
        """x: conv_in's operand - A.pack of the image, icd_vae_ingest's tensor (fp16) or icd_vae_ingest_f32's (fp32) -> (mean, logvar)"""
        w, ws = A.w, A.ws
        s = A.issue(ops.conv3x3, x, (B, H, W), ws["encoder.conv_in.weight"], w["encoder.conv_in.bias"], B * H * W)
        for resnets, down, _ in self.cfg.levels("encoder"):
            for p, _, _ in resnets:
                s = self._resnet(A, p, s, B, H, W)
            if down:
                x, undo = A.raw(s)
                s = A.issue(ops.conv3x3, x, (B, H, W), ws[down + "weight"], w[down + "bias"], B * (H // 2) * (W // 2), stride=2, pad_hi=True, **undo)
                H, W = H // 2, W // 2
        s = self._mid(A, "encoder.mid_block.", s, B, H, W)
        h = A.norm(s, B, H * W, "encoder.conv_norm_out.", True)
        return tuple(ops.conv_out(h, B, H, W, ws[f"encoder.conv_out_{n}.weight"], w[f"encoder.conv_out_{n}.bias"], out_dtype=A.out_dtype, cout=4)
                     for n in ("mean", "logvar"))

    # -- public
    @torch.no_grad()
    def decode(self, z, return_dict=True):
        """z [B,4,h,w] (already / scaling_factor) -> image [B,3,8h,8w] in `self.dtype`."""
        if z.dim() != 4 or z.shape[1] != self.cfg.latent_channels:
            raise ValueError(f"AutoencoderKL.decode: expected [B,{self.cfg.latent_channels},h,w], got {tuple(z.shape)}")
        z = z.to(self.device)
        if z.dtype not in (torch.float16, torch.float32):
            z = z.float()
        A, (H, W) = self._arithmetic(), z.shape[2:]
        outs = []
        for i in range(0, z.shape[0], self.max_chunk):
            c = z[i:i + self.max_chunk].contiguous()
            outs.append(self._decode_body(A, A.pack(c, ones_channel=self.cfg.latent_channels), c.shape[0], H, W))
        img = (outs[0] if len(outs) == 1 else torch.cat(outs)).to(self.dtype)
        return _Out(sample=img) if return_dict else (img,)

    @torch.no_grad()
    def encode(self, x, return_dict=True):
        """image [B,3,H,W] in [-1,1] (H, W multiples of 8) -> latent_dist with `.mean` [B,4,H/8,W/8]."""
        if x.dim() != 4 or x.shape[1] != self.cfg.in_channels or x.shape[2] % 8 or x.shape[3] % 8:
            raise ValueError(f"AutoencoderKL.encode: expected [B,{self.cfg.in_channels},8h,8w], got {tuple(x.shape)}")
        x = x.to(self.device)
        if x.dtype not in (torch.float16, torch.float32):
            x = x.float()
        A, (H, W) = self._arithmetic(), x.shape[2:]
        outs = []
        for i in range(0, x.shape[0], self.max_chunk):
            c = x[i:i + self.max_chunk].contiguous()
            outs.append(self._encode_body(A, A.pack(c), c.shape[0], H, W))
        mean = torch.cat([o[0] for o in outs]).to(self.dtype)
        logvar = torch.cat([o[1] for o in outs]).to(self.dtype)
        dist = LatentDist(mean, logvar)
        return _Out(latent_dist=dist) if return_dict else (dist,)

    @torch.no_grad()
    def encode_images(self, images_u8, size=None, want_bytes=False, return_dict=True, *, rule='load_512', image_dtype=torch.float32):
        """Real images straight into the encoder: uint8 NHWC on the device, [B, H, W, 3] or a list of [H, W, 3] / [b, H, W, 3] tensors
        whose sizes may differ, resized like np.array(PIL.Image.resize((size, size))) (size=None: their own, common, square size) ->
        latent_dist, the bits `encode` gives the host route's `torch.from_numpy(arr).float() / 127.5 - 1` of the resized arrays.
        fp16: icd_vae_ingest writes conv_in's input.  fp32 fidelity: the resized bytes go through the host route's own fp32 values (a
        256-entry table evaluated by that very expression on the host) and _pack32.  The images are ingested size by size and
        encoded in the caller's order, max_chunk at a time like `encode`.  want_bytes: the result also carries the resized bytes as
        ['images'], uint8 [B, size, size, 3].
        rule='image_processor' (fp32 fidelity only; the SDXL route): the same resize, then diffusers' VaeImageProcessor.preprocess,
        `2.0 * (u / 255.0) - 1.0` in fp32 - the bits `encode` gives `preprocess` of the resized PIL images.  icd_vae_ingest_f32 writes
        conv_in's split operand itself: no fp32 image, no lookup, no cast pass.  image_dtype=torch.float16 (this rule only): the bits
        `encode` gives `preprocess(...).half().float()`, the image as a pipeline that runs in fp16 hands it over (diffusers' img2img
        prepare_latents casts to the pipeline's dtype before it upcasts): fp16(v) is the operand's hi half, so its lo half is zero."""
        if rule not in ('load_512', 'image_processor'):
            raise ValueError(f"AutoencoderKL.encode_images: rule must be 'load_512' or 'image_processor', got {rule!r}")
        processor = rule == 'image_processor'
        if image_dtype not in (torch.float16, torch.float32) or (image_dtype != torch.float32 and not processor):
            raise ValueError(f"AutoencoderKL.encode_images: image_dtype is float32, or float16 with rule='image_processor', got {image_dtype}")
        if processor and self.dtype != torch.float32:
            raise ValueError("AutoencoderKL.encode_images: rule='image_processor' needs the fp32-fidelity mode (vae.to(torch.float32)), "
                             f"this VAE is {self.dtype}")
        groups = [images_u8] if isinstance(images_u8, torch.Tensor) else list(images_u8)
        groups = [g[None] if g.dim() == 3 else g for g in groups]
        for g in groups:
            if g.dtype != torch.uint8 or g.dim() != 4 or g.shape[3] != 3 or not g.is_cuda:
                raise ValueError(f"AutoencoderKL.encode_images: expected uint8 [B,H,W,3] on the device, got {g.dtype} {tuple(g.shape)}")
        if not groups:
            raise ValueError("AutoencoderKL.encode_images: no images")
        if size is None:
            sizes = {tuple(g.shape[1:3]) for g in groups}
            size = groups[0].shape[1]
            if len(sizes) != 1 or groups[0].shape[2] != size:
                raise ValueError(f"AutoencoderKL.encode_images: size=None takes square images of one size, got {sorted(sizes)}")
        if size <= 0 or size % 8:
            raise ValueError(f"AutoencoderKL.encode_images: size must be a positive multiple of 8, got {size}")
        f32 = self.dtype == torch.float32
        by_size = {}
        for i, g in enumerate(groups):                           # the images of one size ingest as one batch
            by_size.setdefault(tuple(g.shape[1:3]), []).append(i)
        x8, u8 = {}, {}
        for idx in by_size.values():
            g = groups[idx[0]] if len(idx) == 1 else torch.cat([groups[i] for i in idx])
            if processor:
                a, b = ops.vae_ingest_f32(g.contiguous(), size, want_bytes=want_bytes)
                if image_dtype == torch.float16:
                    a[:, 8:16].zero_()                           # [hi | lo | hi]: an fp16 image has no lo half
            else:
                a, b = ops.vae_ingest(g.contiguous(), size, want_bytes=want_bytes or f32)
            r0 = 0
            for i in idx:
                n = groups[i].shape[0]
                x8[i], u8[i] = a[r0 * size * size:(r0 + n) * size * size], None if b is None else b[r0:r0 + n]
                r0 += n
        one = len(groups) == 1
        x8 = x8[0] if one else torch.cat([x8[i] for i in range(len(groups))])
        u8 = None if u8[0] is None else (u8[0] if one else torch.cat([u8[i] for i in range(len(groups))]))
        B, outs, A = x8.shape[0] // (size * size), [], self._arithmetic()
        if f32 and not processor:
            lut = (torch.arange(256, dtype=torch.uint8).float() / 127.5 - 1).to(self.device)          # the host route's values, exactly
        for i in range(0, B, self.max_chunk):
            n = min(self.max_chunk, B - i)
            if f32 and not processor:
                first = A.pack(lut[u8[i:i + n].long()].permute(0, 3, 1, 2).contiguous())
            else:                                                # the ingest kernel wrote this arithmetic's operand
                first = x8[i * size * size:(i + n) * size * size]
            outs.append(self._encode_body(A, first, n, size, size))
        dist = LatentDist(torch.cat([o[0] for o in outs]).to(self.dtype), torch.cat([o[1] for o in outs]).to(self.dtype))
        if not return_dict:
            return (dist,)
        return _Out(latent_dist=dist, images=u8) if want_bytes else _Out(latent_dist=dist)
