"""The pre-LayerNorm transformer encoder that the CLIP text tower, the CLIP image tower (clip.py) and DINOv2 (dinov2.py) share, and what
the image models (LPIPS, lpips.py, among them) have in common around it.

A tower is a front end (its embeddings), `run_blocks` over the weights that `prepare_block` made, and a back end (final LayerNorm,
pooling, projection).  One block is
    h = LayerNorm(x);  q, k = one fused biased GEMM;  V^T from the transposing GEMM epilogue;  `icd_attention_fused_ex`;
    x <- x + o.w attention + o.b;  h = LayerNorm(x);  x <- x + fc2(act(fc1(h)))
The V bias is folded into the output projection's bias (softmax rows sum to one, also under the causal mask), and so is DINOv2's
LayerScale (`fold_output`).  The residual stream keeps an fp32 twin (icd_gemm_desc.out_f32 + an fp32 `resid`): the 2 x num_hidden_layers
adds x <- x + f(x) accumulate in fp32, the fp16 copy is what LayerNorm and the returned hidden states read (CLIP ViT-L 1.07e-3 -> < 1e-3
against transformers).  fp16 storage, fp32 accumulation.
"""
import torch

from . import ops

ACT = {"quick_gelu": ops.ACT_QUICK_GELU, "gelu": ops.ACT_GELU}
BLOCK_KEYS = ("qk.w", "qk.b", "v.w", "o.w", "o.b", "ln1.w", "ln1.b", "ln2.w", "ln2.b", "fc1.w", "fc1.b", "fc2.w", "fc2.b")


class ModelOutput(tuple):
    """Indexable like the transformers ModelOutput the reference indexes ([0]) with the attributes it reads."""

    def __new__(cls, first, **fields):
        self = super().__new__(cls, (first,) + tuple(v for v in fields.values() if v is not None))
        self.__dict__.update(fields)
        return self


# ------------------------------------------------------------------------------------------------------------ checks
def check_state_dict(sd, want, what):
    """every key of `want` (key -> shape) is in `sd`, with that shape"""
    missing = [k for k in want if k not in sd]
    if missing:
        raise KeyError(f"{what} state dict lacks {len(missing)} tensors, e.g. {missing[:3]}")
    for k, shp in want.items():
        if tuple(sd[k].shape) != tuple(shp):
            raise ValueError(f"{k}: expected shape {tuple(shp)}, got {tuple(sd[k].shape)}")


def check_widths(name, hidden, heads, intermediate, act, extra=()):
    """what the GEMM and attention kernels ask of a tower's widths (`extra`: further widths, such as a projection's)"""
    d = hidden // max(heads, 1)
    if hidden % heads or d > 160 or d % 8 or hidden % 8 or intermediate % 8 or any(e % 8 for e in extra):
        raise ValueError(f"{name}: head dim must be a multiple of 8 and <= 160, widths multiples of 8")
    if act not in ACT:
        raise ValueError(f"{name}: unsupported hidden_act {act!r}")


# ------------------------------------------------------------------------------------------------------------ weights
def half(t, device):
    return t.to(torch.float16).to(device).contiguous()


def full(t, device):
    return t.to(torch.float32).to(device).contiguous()


def fold_output(weight, bias, v_bias=None, lam=None, dtype=torch.float64):
    """(W', b') in `dtype` with W' x + b' = lam * (W (x + v_bias) + b): the V bias (softmax rows sum to one, so it passes through the
    attention unchanged) and a LayerScale vector folded into the Linear that ends the branch.  float64 and one rounding afterwards keep
    the prepared weights independent of which fp32 mat-vec path the host library takes for a tensor's alignment."""
    w, b = weight.to(dtype), bias.to(dtype)
    if v_bias is not None:
        b = w @ v_bias.to(dtype) + b
    if lam is not None:
        w, b = lam.to(dtype)[:, None] * w, lam.to(dtype) * b
    return w, b


def prepare_block(get, names, device, fold_dtype=torch.float64, lam1=None, lam2=None):
    """The tensors of one block under BLOCK_KEYS.  `get(key)` is the checkpoint's tensor in fp32 on the host, or None for a bias that
    the checkpoint does not have (DINOv2 without qkv_bias); `names` maps q, k, v, out, norm1, norm2, fc1, fc2 to its module paths;
    lam1 / lam2 are the LayerScale vectors behind the attention and the MLP, where the model has them."""
    weight = lambda n: get(names[n] + ".weight")

    def bias(n):
        b = get(names[n] + ".bias")
        return torch.zeros(weight(n).shape[0]) if b is None else b
    wo, bo = fold_output(weight("out"), bias("out"), bias("v"), lam1, fold_dtype)
    w2, b2 = fold_output(weight("fc2"), bias("fc2"), None, lam2, fold_dtype)
    halves = {"qk.w": torch.cat([weight("q"), weight("k")]), "v.w": weight("v"), "o.w": wo, "fc1.w": weight("fc1"), "fc2.w": w2}
    fulls = {"qk.b": torch.cat([bias("q"), bias("k")]), "o.b": bo, "ln1.w": weight("norm1"), "ln1.b": bias("norm1"),
             "ln2.w": weight("norm2"), "ln2.b": bias("norm2"), "fc1.b": bias("fc1"), "fc2.b": b2}
    return {k: half(halves[k], device) if k in halves else full(fulls[k], device) for k in BLOCK_KEYS}


# ------------------------------------------------------------------------------------------------------------ the blocks
def run_blocks(w, prefixes, x, x32, B, T, heads, eps, act, causal, hidden_states=None, norm_f32=False, split_qk=False):
    """fp16 stream x [B * T, C] through the blocks whose weights are w[prefix + key] -> (x, its fp32 twin).  x32 is the twin where the
    front end made one, or None: the first add then reads the fp16 stream.  The stream after each block is appended to `hidden_states`.
    norm_f32 (needs x32): the LayerNorms read the fp32 twin (icd_layernorm_f32), not its fp16 copy - one rounding fewer in front of
    every projection.  split_qk (not with causal): q and k leave their GEMM as fp16 + error carry (icd_gemm_desc.out_carry) and the
    scores are taken from both parts (icd_attention_probs_split, then P.V as a batched GEMM) - the logits lose the rounding of q and k.
    Both are what the BLIP image tower's peaked attention rows need to stay under 1e-3 over 24 blocks."""
    C = x.shape[1]
    d, ld = C // heads, (T + 7) // 8 * 8
    if norm_f32 and x32 is None:
        raise ValueError("run_blocks: norm_f32 needs the fp32 twin of the stream")
    if split_qk and causal:
        raise ValueError("run_blocks: split_qk has no causal form")

    def norm(x, x32, k):
        if norm_f32:
            return ops.layernorm_f32(x32, w[k + ".w"], w[k + ".b"], eps, want32=False)[0]
        return ops.layernorm(x, w[k + ".w"], w[k + ".b"], eps)

    def add(f, wk, bk, x, x32):
        n32 = torch.empty(x.shape, device=x.device, dtype=torch.float32)
        return ops.gemm(f, w[wk], w[bk], resid=x if x32 is None else x32, out32=n32), n32
    for p in prefixes:
        h = norm(x, x32, p + "ln1")
        vt = ops.project_vt(h, w[p + "v.w"], B, T, ld)
        if split_qk:
            carry = torch.empty((x.shape[0], 2 * C), device=x.device, dtype=torch.uint8)
            qk = ops.gemm(h, w[p + "qk.w"], w[p + "qk.b"], out_carry=carry)
            probs = ops.attention_probs(qk[:, :C], qk[:, C:], B, heads, T, T, d, d ** -0.5, ld=ld, q_carry=carry[:, :C], k_carry=carry[:, C:])
            o = ops.attention_apply(probs, vt, B, heads, T, d)
        else:
            qk = ops.gemm(h, w[p + "qk.w"], w[p + "qk.b"])
            o = ops.attention_fused(qk[:, :C], qk[:, C:], vt, B, heads, T, T, d, d ** -0.5, causal=causal)
        x, x32 = add(o, p + "o.w", p + "o.b", x, x32)
        h = norm(x, x32, p + "ln2")
        f = ops.activation(ops.gemm(h, w[p + "fc1.w"], w[p + "fc1.b"]), ACT[act])
        x, x32 = add(f, p + "fc2.w", p + "fc2.b", x, x32)
        if hidden_states is not None:
            hidden_states.append(x)
    return x, x32


# ------------------------------------------------------------------------------------------------------------ images
def images_to_device(images, device):
    """PIL images / numpy uint8 HWC arrays (one size) / a uint8 NHWC tensor -> contiguous uint8 [B, H, W, 3] on `device`.  A tensor that
    already lives there is returned as it is: nothing is copied to the host."""
    import numpy as np
    if isinstance(images, torch.Tensor):
        t = images
    else:
        if not isinstance(images, (list, tuple)):
            images = [images]
        arrs = []
        for im in images:
            if isinstance(im, torch.Tensor):
                im = im.cpu().numpy()
            elif not isinstance(im, np.ndarray):
                im = np.array(im.convert("RGB"))                # PIL: do_convert_rgb of the processor
            arrs.append(im)
        if len({a.shape for a in arrs}) != 1:
            raise ValueError("images_to_device: images of several sizes; pass them in groups of one size")
        t = torch.from_numpy(np.stack(arrs))
    if t.dtype != torch.uint8 or t.dim() != 4 or t.shape[3] != 3:
        raise ValueError(f"images must be uint8 [B, H, W, 3], got {t.dtype} {tuple(t.shape)}")
    return t.to(device).contiguous()


def image_batch_to_device(images, device):
    """images_to_device for the models that also take a stacked uint8 NHWC ndarray as a batch (images_to_device itself takes an ndarray
    for ONE image, and the CLIP and DINOv2 towers, which call it directly, refuse a stacked one)."""
    import numpy as np
    if isinstance(images, np.ndarray) and images.ndim == 4:
        images = torch.from_numpy(np.ascontiguousarray(images))
    return images_to_device(images, device)


def image_size(im):
    """(height, width) of a PIL image or an HWC array or tensor"""
    return tuple(im.shape[:2]) if hasattr(im, "shape") else im.size[::-1]


def mixed_sizes(images):
    """a list that holds images of several sizes"""
    return isinstance(images, (list, tuple)) and len({image_size(im) for im in images}) > 1


def run_by_size(n, key, run):
    """Items 0 .. n - 1 grouped by key(i); run(indices) -> a device tensor with one row per index, once per group; the rows come back in
    the caller's order.  (The models take one image size per batch; a list from the caller may mix them.)"""
    groups = {}
    for i in range(n):
        groups.setdefault(key(i), []).append(i)
    if len(groups) <= 1:
        return run(list(range(n)))
    out = None
    for idx in groups.values():
        rows = run(idx)
        out = rows.new_empty((n,) + tuple(rows.shape[1:])) if out is None else out
        out[torch.as_tensor(idx, device=rows.device)] = rows
    return out
