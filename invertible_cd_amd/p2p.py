"""Prompt-to-prompt attention-control plugin for the native UNet (API mirror of the reference's utils/p2p.py).

Same module globals (NUM_DDIM_STEPS / tokenizer / device / LOW_RESOURCE / MAX_NUM_WORDS, utils/p2p.py:9-13), same classes
(AttentionStore, AttentionReplace, AttentionRefine, AttentionReweight, LocalBlend, EmptyControl, SpatialReplace) and the
same entry points (register_attention_control, make_controller, get_equalizer, get_word_inds,
get_time_words_attention_alpha).  Semantics are pinned by golden vectors captured from the reference
(tests/golden/p2p.npz, tests/test_p2p_golden.py).

What is different underneath: the reference monkey-patches every diffusers `Attention.forward` (utils/p2p.py:291-386).
Here `register_attention_control` hands the controller to the native executor, which calls back (C ABI hook,
include/icd_amd.h) once per Attention module in module-execution order; `HookAdapter` decides per layer whether the
probabilities must be materialised at all:
  * layers the controller does not read or edit (`needs_probs` False, e.g. N > 32^2 self-attention for every shipped
    controller, utils/p2p.py:147,184-188) run the fused flash kernel and only tick the controller's counters;
  * when the sampler eliminated the dead unconditional half of the CFG batch (utils/generation.py:247-251 discards it
    when w_embed_dim > 0) the controller's `forward` - which in the reference only ever sees the conditional half,
    utils/p2p.py:106-107 - is applied to the whole (cond-only) tensor.  The SDXL sampler (generation_sdxl.sample_deterministic
    with `controller=`) always runs this layout: its batch [source, edit_1, ...] has no unconditional half at all.

Who decides what on a materialised layer.  The controller says what it needs: every editing controller is a `PromptGroupEdit`, G prompt
groups of P on the conditional samples (`layout`: one reference-shaped controller is (1, P), a `ControllerBatch` (G, P)), with a step's
packed cross-attention operators (`cross_edit_operator`), its self-replace window (`self_window`) and, as an AttentionStore, the store
tensor that the layer's map goes to (`store_target`).  The adapter plans (`HookAdapter.plan`, written once, for G groups) which of these
the probability kernel's epilogue takes over for this batch layout and layer geometry: one pass over P instead of three
(`controller.fused_epilogue = False`, `controller.cond_rows_only = False`: the A/B switches, same bits).  The kernel executes.  The
`LayerCall` record carries the plan from `query` to `probs_ready`, which tells the controller what is already done (`kernel_did`):
`forward` leaves that edit alone and `between_steps` skips those entries.  The rest runs as one launch for all groups where the rows
are the kernel's (`PromptGroupEdit.edit_rows`, `LocalBlend.blend_groups`), else as the torch expressions that the goldens pin.
"""
import abc
from typing import Dict, List, Optional, Tuple, Union

import numpy as np
import torch
import torch.nn.functional as nnf

from . import seq_aligner

MAX_NUM_WORDS = 77
LOW_RESOURCE = False
NUM_DDIM_STEPS = 50
device = "cuda"
tokenizer = None


# ------------------------------------------------------------------------------------------- latent blending
class LocalBlend:
    """Word-localised latent blending from the accumulated cross-attention maps (utils/p2p.py:18-70).

    The reference reads down_cross[2:4] + up_cross[:3] as 16 x 16 maps against a 64 x 64 latent.  Those are exactly the stored
    cross-attention maps of the down and up places whose side is a quarter of the latent's, and that is the rule here (`select_maps`):
    SD1.5 at 64 x 64 latents gives the same five maps in the same order; SDXL at 128 x 128 latents gives its 1024-query layers as
    32 x 32 maps, 20 down + 30 up (the mid block works at an eighth and stays out, as in SD1.5)."""

    def __init__(self, prompts: List[str], words, substruct_words=None, start_blend=0.2, th=(.3, .3)):
        self.alpha_layers = self._word_mask(prompts, words).to(device)
        self.substruct_layers = None if substruct_words is None else self._word_mask(prompts, substruct_words).to(device)
        self.start_blend = int(start_blend * NUM_DDIM_STEPS)
        self.counter = 0
        self.th = th
        self._device_terms = {}        # blend_groups' cache for this LocalBlend alone

    @staticmethod
    def _word_mask(prompts, words):
        mask = torch.zeros(len(prompts), 1, 1, 1, 1, MAX_NUM_WORDS)
        for i, (prompt, ws) in enumerate(zip(prompts, words)):
            for w in ([ws] if isinstance(ws, str) else ws):
                mask[i, :, :, :, :, get_word_inds(prompt, w, tokenizer)] = 1
        return mask

    @staticmethod
    def select_maps(attention_store, x_t):
        """(maps, (rows, cols)): the stored down / up cross-attention maps at a quarter of the latent's side, in store order."""
        rows, cols = x_t.shape[2] // 4, x_t.shape[3] // 4
        down, up = attention_store["down_cross"], attention_store["up_cross"]
        ref = down[2:4] + up[:3]
        if len(down) <= 4 and len(up) <= 6 and ref and all(m.shape[1] == rows * cols for m in ref):
            # a store no larger than SD1.5's (4 down + 6 up maps kept): the reference's own positions.  On SD1.5 they ARE the quarter-side
            # maps; a smaller store (the golden walk of tests/golden/p2p.npz keeps three 16 x 16 maps per place) is read as the reference
            # reads it, position by position, so every vector captured from the reference stays what it was.
            return ref, (rows, cols)
        maps = [m for m in down + up if m.shape[1] == rows * cols]
        if rows * cols == 0 or not maps:
            raise ValueError(f"LocalBlend: the store holds no down / up cross-attention map of {rows} x {cols} queries (a quarter of the "
                             f"{x_t.shape[2]} x {x_t.shape[3]} latent's side); stored: "
                             f"{sorted({m.shape[1] for m in attention_store['down_cross'] + attention_store['up_cross']})}")
        return maps, (rows, cols)

    @staticmethod
    def _on_device(x_t, layers, side=(16, 16)):
        """The HIP kernels take the accumulated store tensors as they are: fp16 on the GPU, [P*heads, res*res, 77] with evenly strided
        rows, res <= 32, up to 64 layers.  Anything else (CPU goldens, foreign dtypes, non-square maps) takes the torch expression below."""
        n = side[0] * side[1]
        if not (x_t.is_cuda and x_t.dim() == 4 and x_t.dtype in (torch.float16, torch.float32) and side[0] == side[1] and 0 < n <= 1024):
            return False
        for m in layers:
            if not (m.is_cuda and m.dtype == torch.float16 and m.dim() == 3 and m.shape[1] == n and m.shape[2] == MAX_NUM_WORDS
                    and m.stride(2) == 1 and m.stride(1) == layers[0].stride(1) and m.stride(0) == n * m.stride(1)):
                return False
        return len(layers) <= 64

    def get_mask(self, maps, alpha, use_pool, x_t):
        """Word-weighted mean over layers x heads of the maps -> (3x3 max-pool) -> nearest resize to the latent ->
        per-prompt max normalisation -> threshold; every prompt's mask is OR-ed with the base prompt's (utils/p2p.py:20-31)."""
        heat = (maps * alpha).sum(-1).mean(1)                              # [P, 1, res, res]
        if use_pool:
            heat = nnf.max_pool2d(heat, kernel_size=3, stride=1, padding=1)
        heat = nnf.interpolate(heat, size=(x_t.shape[2:]))
        heat = heat / heat.amax(dim=(2, 3), keepdim=True)
        on = heat.gt(self.th[1 - int(use_pool)])
        return on[:1] + on

    def __call__(self, x_t, attention_store):
        """`x_t[e] <- x_t[0] + mask[e] * (x_t[e] - x_t[0])` from the accumulated quarter-side cross-attention maps
        (utils/p2p.py:33-44: down_cross[2:4] + up_cross[:3] at 16 x 16)."""
        return self.blend(x_t, attention_store) if self.due() else x_t

    def due(self):                                               # advance the step counter: is this step past start_blend?
        self.counter += 1
        return self.counter > self.start_blend

    @staticmethod
    def blend_groups(lbs, active, x_t, layers, side, cache):
        """The blend of G prompt groups (`lbs`: a LocalBlend or None each, a lone LocalBlend is the one-element list; `active`: which of
        them blend at this step) in two HIP launches: word-weighted mean of the maps; pool, normalise, threshold, OR with the base prompt's
        mask, substruct words, nearest resize and the blend itself.  None where the torch expression has to run.  `cache`: the caller's."""
        P = x_t.shape[0] // len(lbs)
        if not (LocalBlend._on_device(x_t, layers, side) and all(lb is None or lb.alpha_layers.shape[0] == P for lb in lbs)):
            return None
        dev = x_t.device
        if str(dev) not in cache:
            def words(mask):                                     # a group's [P, 77] word mask; zero where it has none
                return torch.zeros(P, MAX_NUM_WORDS, device=dev) if mask is None else mask.reshape(P, MAX_NUM_WORDS).to(dev, torch.float32)
            has_sub = [lb is not None and lb.substruct_layers is not None for lb in lbs]
            sub = (torch.cat([words(lb.substruct_layers if h else None) for lb, h in zip(lbs, has_sub)]), has_sub) if any(has_sub) else None
            cache[str(dev)] = (torch.cat([words(None if lb is None else lb.alpha_layers) for lb in lbs]), sub,
                               [0.0 if lb is None else lb.th[0] for lb in lbs], [0.0 if lb is None else lb.th[1] for lb in lbs])
        alpha, sub, th_pool, th_sub = cache[str(dev)]
        from . import ops
        return ops.local_blend_groups(layers, alpha, sub, th_pool, th_sub, active, x_t.contiguous(), len(lbs), res=side[0])

    def blend(self, x_t, attention_store):
        """The blend itself, past start_blend (what __call__ does after advancing its counter)."""
        layers, side = self.select_maps(attention_store, x_t)
        out = self.blend_groups([self], [True], x_t, layers, side, self._device_terms)
        if out is not None:
            return out
        maps = torch.cat([m.reshape(self.alpha_layers.shape[0], -1, 1, side[0], side[1], MAX_NUM_WORDS) for m in layers], dim=1)
        mask = self.get_mask(maps, self.alpha_layers, True, x_t)
        if self.substruct_layers is not None:
            mask = mask * ~self.get_mask(maps, self.substruct_layers, False, x_t)
        base = x_t[:1]
        return base + mask.float() * (x_t - base)


# ------------------------------------------------------------------------------------------- controllers
class EmptyControl:
    def step_callback(self, x_t):
        return x_t

    def between_steps(self):
        return

    def needs_probs(self, is_cross, n_queries, place_in_unet):
        return False

    def __call__(self, attn, is_cross: bool, place_in_unet: str):
        return attn


class AttentionControl(abc.ABC):
    """Counter logic of utils/p2p.py:85-122.  `forward` receives the conditional rows only."""

    def __init__(self):
        self.cur_step = 0
        self.num_att_layers = -1
        self.cur_att_layer = 0

    def step_callback(self, x_t):
        return x_t

    def between_steps(self):
        return

    @property
    def num_uncond_att_layers(self):
        return self.num_att_layers if LOW_RESOURCE else 0

    @abc.abstractmethod
    def forward(self, attn, is_cross: bool, place_in_unet: str):
        raise NotImplementedError

    def needs_probs(self, is_cross, n_queries, place_in_unet):
        """May `forward` read or modify the probabilities of such a layer?  Unknown subclasses: always."""
        return True

    def _advance(self):
        self.cur_att_layer += 1
        if self.cur_att_layer == self.num_att_layers + self.num_uncond_att_layers:
            self.cur_att_layer = 0
            self.cur_step += 1
            self.between_steps()

    def __call__(self, attn, is_cross: bool, place_in_unet: str):
        """CFG-doubled layout [uncond rows ; cond rows] (utils/p2p.py:101-113): edit the second half in place."""
        if self.cur_att_layer >= self.num_uncond_att_layers:
            if LOW_RESOURCE:
                attn = self.forward(attn, is_cross, place_in_unet)
            else:
                half = attn.shape[0] // 2
                attn[half:] = self.forward(attn[half:], is_cross, place_in_unet)
        self._advance()
        return attn

    def call_cond_only(self, attn, is_cross: bool, place_in_unet: str):
        """The whole tensor is the conditional half (dead unconditional rows were never computed)."""
        if self.cur_att_layer >= self.num_uncond_att_layers:
            new = self.forward(attn, is_cross, place_in_unet)
            if new is not attn:
                attn.copy_(new)
        self._advance()
        return attn

    def tick(self):
        """A layer whose probabilities this controller neither reads nor edits was executed (fused kernel)."""
        self._advance()

    def reset(self):
        self.cur_step = 0
        self.cur_att_layer = 0


class SpatialReplace(EmptyControl):
    def __init__(self, stop_inject: float):
        super().__init__()
        self.stop_inject = int((1 - stop_inject) * NUM_DDIM_STEPS)

    def step_callback(self, x_t):
        if self.cur_step < self.stop_inject:
            x_t = x_t[:1].expand(x_t.shape[0], *x_t.shape[1:])
        return x_t


class AttentionStore(AttentionControl):
    """Keeps (views of) the conditional probabilities of every layer with <= 32^2 queries and sums them over steps
    (utils/p2p.py:138-173)."""

    STORE_MAX_QUERIES = 32 ** 2

    def __init__(self):
        super().__init__()
        self.step_store = self.get_empty_store()
        self.attention_store = {}
        self.layout = None             # (G, P): the rows are G prompt groups of P that an edit couples (PromptGroupEdit); None: only stored
        self.kernel_edit = False       # kernel_did: the probability kernel has applied this step's edit to the layer being handed over
        self._fused_acc = set()        # kernel_did: (key, index) of this step's maps the probability kernel has added to attention_store
        self._acc_geometry = {}        # store_target: (key, index) -> (store tensor, can the kernel add to it), checked once per tensor

    @staticmethod
    def get_empty_store():
        return {f"{place}_{kind}": [] for kind in ("cross", "self") for place in ("down", "mid", "up")}

    def needs_probs(self, is_cross, n_queries, place_in_unet):
        return (self.layout is not None and is_cross) or n_queries <= self.STORE_MAX_QUERIES

    def forward(self, attn, is_cross: bool, place_in_unet: str):
        if attn.shape[1] <= self.STORE_MAX_QUERIES:
            self.step_store[f"{place_in_unet}_{'cross' if is_cross else 'self'}"].append(attn)
        return attn

    def between_steps(self):
        if not self.attention_store:
            self.attention_store = self.step_store
        else:
            pairs = [(t, self.step_store[key][i]) for key, acc in self.attention_store.items() for i, t in enumerate(acc)
                     if (key, i) not in self._fused_acc]       # those the probability kernel's epilogue has added (icd_probs_epilogue.acc)
            if pairs and all(t.is_cuda and t.dtype == torch.float16 and t.is_contiguous() and s.is_cuda and s.dtype == torch.float16
                             and s.is_contiguous() and t.shape == s.shape and t.data_ptr() % 16 == 0 and s.data_ptr() % 16 == 0
                             for t, s in pairs):
                from . import ops                  # one launch for all stored maps (icd_accumulate_multi), same rounding as `t += s`
                ops.accumulate_multi([t for t, _ in pairs], [s for _, s in pairs])
            else:
                for t, s in pairs:
                    t += s
        self.step_store = self.get_empty_store()
        self._fused_acc = set()

    def get_average_attention(self):
        return {key: [t / self.cur_step for t in ts] for key, ts in self.attention_store.items()}

    def store_target(self, key, shape, ld):
        """(index, tensor) of attention_store that the next map of `key` is added to, where the probability kernel can do that itself
        (fp16 on the GPU, `shape` with rows of `ld`, 16-byte aligned); else None: between_steps adds it."""
        idx = len(self.step_store[key])
        acc = self.attention_store.get(key, ())
        if idx >= len(acc):
            return None
        t = acc[idx]
        ok = self._acc_geometry.get((key, idx))
        if ok is None or ok[0] is not t:
            ok = self._acc_geometry[(key, idx)] = (t, t.is_cuda and t.dtype == torch.float16 and tuple(t.shape) == shape
                                                   and t.stride() == (shape[1] * ld, ld, 1) and t.data_ptr() % 16 == 0)
        return (idx, t) if ok[1] else None

    def kernel_did(self, edit, acc_key=None):
        """HookAdapter around the controller call of one layer: the probability kernel has applied this step's edit to the probabilities
        (`edit`) and added them to attention_store[key][index] (`acc_key`).  `kernel_did(False)` once the call is over."""
        self.kernel_edit = edit
        if acc_key is not None:
            self._fused_acc.add(acc_key)

    def reset(self):
        super().reset()
        self.step_store = self.get_empty_store()
        self.attention_store = {}
        self.kernel_edit = False
        self._fused_acc = set()
        self._acc_geometry = {}


class PromptGroupEdit(AttentionStore):
    """The prompt-group view of an edit: the conditional rows are G independent groups of P prompts [base | edits] x heads, group-major.
    A subclass states its `layout`, `self_window(step)` (True, False, or None when the groups disagree), `_edit_operator(step, dev)` and
    the torch expressions `edit_rows_torch`."""

    def __init__(self, layout):
        super().__init__()
        self.layout = layout
        self._edit_ops = {}            # (step, device) -> cross_edit_operator

    def cross_edit_operator(self, step, dev):
        """The packed operators (ops.p2p_pack_operator) of  a_t * replace_cross_attention(base, cur) + (1 - a_t) * cur  at `step`, ordered
        [group][edit] ([G*(P-1), 96, 80] fp16 / [G*(P-1), 96] fp32), cached on `dev`."""
        key = (int(step), str(dev))
        if key not in self._edit_ops:
            self._edit_ops[key] = self._edit_operator(step, dev)
        return self._edit_ops[key]

    def forward(self, attn, is_cross: bool, place_in_unet: str):
        super().forward(attn, is_cross, place_in_unet)          # stores a VIEW (of all groups' rows): the stored tensor sees the edit below
        if self.layout is None or self.kernel_edit:             # nothing to edit, or the probability kernel's epilogue has done it already
            return attn
        return self.edit_rows(attn, is_cross, place_in_unet)

    def edit_rows(self, attn, is_cross: bool, place_in_unet: str):
        """This step's edit of the conditional rows (forward after storing the view)."""
        G, P = self.layout
        if is_cross and attn.is_cuda and attn.shape[0] % (G * P) == 0:
            from . import ops                                    # fused in-place HIP kernel (matrix cores, fp32 accumulate), all groups
            if ops.p2p_cross_edit_supported(attn):               # the executor's 80-column rows; else the torch path
                At, Dp = self.cross_edit_operator(self.cur_step, attn.device)
                return ops.p2p_cross_edit_groups(attn, G, P, At, Dp)
        return self.edit_rows_torch(attn, is_cross, place_in_unet)


class AttentionControlEdit(PromptGroupEdit, abc.ABC):
    """Cross/self attention injection between a base prompt (row group 0) and its edits (utils/p2p.py:176-221)."""

    def __init__(self, prompts, num_steps: int, cross_replace_steps, self_replace_steps, local_blend: Optional[LocalBlend]):
        super().__init__((1, len(prompts)))
        self.batch_size = len(prompts)
        self.cross_replace_alpha = get_time_words_attention_alpha(prompts, num_steps, cross_replace_steps, tokenizer).to(device)
        if type(self_replace_steps) is float:
            self_replace_steps = 0, self_replace_steps
        self.num_self_replace = int(num_steps * self_replace_steps[0]), int(num_steps * self_replace_steps[1])
        self.local_blend = local_blend

    def step_callback(self, x_t):
        return x_t if self.local_blend is None else self.local_blend(x_t, self.attention_store)

    def replace_self_attention(self, attn_base, att_replace, place_in_unet):
        if att_replace.shape[2] > self.STORE_MAX_QUERIES:
            return att_replace
        return attn_base.unsqueeze(0).expand(att_replace.shape[0], *attn_base.shape)

    @abc.abstractmethod
    def replace_cross_attention(self, attn_base, att_replace):
        raise NotImplementedError

    # ---- the same edit as one linear operator per step (device path: ops.p2p_cross_edit_groups, csrc/p2p.hip) -------------
    def cross_edit_terms(self, dev):
        """(A0 [P-1, T, T], D0 [P-1, T]) fp32 on `dev` with  replace_cross_attention(base, cur)[b] == base . A0[b] + D0[b] * cur[b]."""
        raise NotImplementedError

    def _edit_operator(self, step, dev):
        A0, D0 = self.cross_edit_terms(dev)  # built on `dev` with torch ops: no host round trip (a sync inside the UNet's hook
        a = self.cross_replace_alpha[step].reshape(self.batch_size - 1, -1).to(dev, torch.float32)   # callbacks would serialise CPU and GPU)
        from . import ops
        return ops.p2p_pack_operator(A0 * a[:, None, :], D0 * a + (1.0 - a))

    def self_window(self, step):
        return self.num_self_replace[0] <= step < self.num_self_replace[1]

    def edit_rows_torch(self, attn, is_cross: bool, place_in_unet: str):
        if not (is_cross or self.self_window(self.cur_step)):
            return attn
        heads = attn.shape[0] // self.batch_size
        grouped = attn.reshape(self.batch_size, heads, *attn.shape[1:])
        base, edits = grouped[0], grouped[1:]
        if is_cross:
            a = self.cross_replace_alpha[self.cur_step]
            grouped[1:] = self.replace_cross_attention(base, edits) * a + (1 - a) * edits
        else:
            grouped[1:] = self.replace_self_attention(base, edits, place_in_unet)
        return grouped.reshape(self.batch_size * heads, *grouped.shape[2:])


class AttentionReplace(AttentionControlEdit):
    def __init__(self, prompts, num_steps: int, cross_replace_steps, self_replace_steps, local_blend: Optional[LocalBlend] = None):
        super().__init__(prompts, num_steps, cross_replace_steps, self_replace_steps, local_blend)
        self.mapper = seq_aligner.get_replacement_mapper(prompts, tokenizer).to(device)

    def replace_cross_attention(self, attn_base, att_replace):
        return torch.einsum("hpw,bwn->bhpn", attn_base, self.mapper.to(attn_base.dtype))

    def cross_edit_terms(self, dev):
        m = self.mapper.to(dev, torch.float32)
        return m, torch.zeros(m.shape[0], m.shape[2], device=dev)


class AttentionRefine(AttentionControlEdit):
    def __init__(self, prompts, num_steps: int, cross_replace_steps, self_replace_steps, local_blend: Optional[LocalBlend] = None):
        super().__init__(prompts, num_steps, cross_replace_steps, self_replace_steps, local_blend)
        mapper, alphas = seq_aligner.get_refinement_mapper(prompts, tokenizer)
        self.mapper = mapper.to(device)
        self.alphas = alphas.to(device).reshape(alphas.shape[0], 1, 1, alphas.shape[1])

    def replace_cross_attention(self, attn_base, att_replace):
        gathered = attn_base[:, :, self.mapper].permute(2, 0, 1, 3)
        return gathered * self.alphas + att_replace * (1 - self.alphas)

    def cross_edit_terms(self, dev):
        idx = self.mapper.to(dev, torch.int64)                                 # [P-1, T]; -1 indexes the last token
        al = self.alphas.reshape(idx.shape[0], -1).to(dev, torch.float32)     # [P-1, T]
        T = idx.shape[1]
        A0 = torch.zeros(idx.shape[0], T, T, device=dev)
        A0.scatter_(1, (idx % T)[:, None, :], al[:, None, :])                 # A0[b, idx[b, n], n] = alphas[b, n]
        return A0, 1.0 - al


class AttentionReweight(AttentionControlEdit):
    def __init__(self, prompts, num_steps: int, cross_replace_steps, self_replace_steps, equalizer,
                 local_blend: Optional[LocalBlend] = None, controller: Optional[AttentionControlEdit] = None):
        super().__init__(prompts, num_steps, cross_replace_steps, self_replace_steps, local_blend)
        self.equalizer = equalizer.to(device)
        self.prev_controller = controller
        self.attn = []

    def replace_cross_attention(self, attn_base, att_replace):
        if self.prev_controller is not None:
            attn_base = self.prev_controller.replace_cross_attention(attn_base, att_replace)
        return attn_base[None, :, :, :] * self.equalizer[:, None, None, :]

    def cross_edit_terms(self, dev):
        eq = self.equalizer.to(dev, torch.float32)                            # [P-1, T]
        if self.prev_controller is not None:
            A0, D0 = self.prev_controller.cross_edit_terms(dev)
        else:
            T = eq.shape[1]
            A0, D0 = torch.eye(T, device=dev).expand(eq.shape[0], T, T), torch.zeros(eq.shape[0], T, device=dev)
        return A0 * eq[:, None, :], D0 * eq


def make_controller(prompts: List[str], is_replace_controller: bool, cross_replace_steps, self_replace_steps,
                    blend_words=None, equilizer_params=None) -> AttentionControlEdit:
    """utils/p2p.py:272-289 (argument names kept, incl. `equilizer_params`)."""
    lb = None if blend_words is None else LocalBlend(prompts, blend_words, start_blend=0.0, th=(0.3, 0.3))
    cls = AttentionReplace if is_replace_controller else AttentionRefine
    controller = cls(prompts, NUM_DDIM_STEPS, cross_replace_steps=cross_replace_steps, self_replace_steps=self_replace_steps,
                     local_blend=lb)
    if equilizer_params is not None:
        eq = get_equalizer(prompts[1], equilizer_params["words"], equilizer_params["values"])
        controller = AttentionReweight(prompts, NUM_DDIM_STEPS, cross_replace_steps=cross_replace_steps,
                                       self_replace_steps=self_replace_steps, equalizer=eq, local_blend=lb, controller=controller)
    return controller


# ------------------------------------------------------------------------------------------- batched editing
class ControllerBatch(PromptGroupEdit):
    """One controller per image for a UNet batch of G independent prompt groups [g0: P samples | g1: P samples | ...] (batched
    editing: many images edited in one call instead of a stream of batch-P calls).

    Members are the reference-shaped controllers of make_controller (AttentionReplace / Refine / Reweight) with the same number of
    prompts P, or plain AttentionStores.  The batch keeps ONE store tensor per layer (all groups' rows: the probability kernel's
    store epilogue keeps working); after every step each member's attention_store holds views of its own rows and its counters
    (cur_step, cur_att_layer, LocalBlend.counter) stand where a run of its own would have left them, so get_average_attention() and
    the LocalBlend of every image work per image."""

    EDIT_TYPES = ("AttentionReplace", "AttentionRefine", "AttentionReweight")

    def __init__(self, controllers):
        members = list(controllers)
        if not members:
            raise ValueError("ControllerBatch needs at least one controller")
        if all(type(c).__name__ in self.EDIT_TYPES and type(c).__module__ == __name__ for c in members):
            sizes = {c.batch_size for c in members}
            if len(sizes) != 1:
                raise ValueError(f"ControllerBatch: every group must have the same number of prompts (got {sorted(sizes)}); split by P")
            self.n_prompts, self.is_edit = sizes.pop(), True
        elif all(type(c) is AttentionStore for c in members):
            self.n_prompts, self.is_edit = None, False
        else:
            raise ValueError("ControllerBatch: members must all be make_controller edit controllers or all plain AttentionStores, "
                             f"got {sorted({type(c).__name__ for c in members})}")
        self.members = members
        self._blend_terms = {}         # LocalBlend.blend_groups' cache for the members' LocalBlends
        super().__init__((len(members), self.n_prompts) if self.is_edit else None)

    @property
    def n_groups(self):
        return len(self.members)

    @property
    def num_att_layers(self):
        return self._num_att_layers

    @num_att_layers.setter
    def num_att_layers(self, n):
        self._num_att_layers = n
        for m in self.members:
            m.num_att_layers = n

    def self_window(self, step):
        w = {m.self_window(step) for m in self.members}
        return w.pop() if len(w) == 1 else None

    def _edit_operator(self, step, dev):
        ops_ = [m.cross_edit_operator(step, dev) for m in self.members]
        return torch.cat([a for a, _ in ops_]).contiguous(), torch.cat([d for _, d in ops_]).contiguous()

    def edit_rows_torch(self, attn, is_cross: bool, place_in_unet: str):
        rows = attn.shape[0] // self.n_groups
        for g, m in enumerate(self.members):                     # per group: the member's own edit on its own rows
            v = attn[g * rows:(g + 1) * rows]
            new = m.edit_rows(v, is_cross, place_in_unet)
            if new is not v and new.data_ptr() != v.data_ptr():
                v.copy_(new)
        return attn

    def _advance(self):
        super()._advance()
        for m in self.members:
            m.cur_att_layer, m.cur_step = self.cur_att_layer, self.cur_step

    def between_steps(self):
        super().between_steps()
        G = self.n_groups
        for g, m in enumerate(self.members):                     # every member's store: views of its own rows of the batch's tensors
            m.attention_store = {key: [t[g * (t.shape[0] // G):(g + 1) * (t.shape[0] // G)] for t in ts]
                                 for key, ts in self.attention_store.items()}
            m.step_store = m.get_empty_store()

    def reset(self):
        super().reset()
        for m in self.members:
            m.reset()

    def step_callback(self, x_t):
        if not self.is_edit:
            return x_t
        G, P = self.n_groups, self.n_prompts
        if x_t.shape[0] != G * P:
            raise ValueError(f"ControllerBatch.step_callback: {x_t.shape[0]} latents for {G} groups of {P} prompts")
        lbs = [m.local_blend for m in self.members]
        active = [lb is not None and lb.due() for lb in lbs]     # each member's LocalBlend counter advances as in a run of its own
        if not any(active):
            return x_t
        layers, side = LocalBlend.select_maps(self.attention_store, x_t)
        out = LocalBlend.blend_groups(lbs, active, x_t, layers, side, self._blend_terms)
        if out is not None:
            return out
        return torch.cat([m.local_blend.blend(xg, m.attention_store) if on else xg
                          for m, on, xg in zip(self.members, active, x_t.split(P))])


# ------------------------------------------------------------------------------------------- registration
class DummyController:
    """What the reference installs for `controller=None` (utils/p2p.py:356-365)."""

    def __init__(self):
        self.num_att_layers = 0

    def __call__(self, *args):
        return args[0]


def register_attention_control(model, controller):
    """Attach `controller` to `model.unet` (utils/p2p.py:291-386).  Sets controller.num_att_layers to the number of
    Attention modules (32 for SD1.5, 140 for SDXL), exactly as the reference's module walk does."""
    if controller is None:
        controller = DummyController()
    unet = model.unet
    if hasattr(unet, "num_attention_layers"):
        unet.attn_controller = None if isinstance(controller, DummyController) else controller
        controller.num_att_layers = unet.num_attention_layers
    else:        # a foreign UNet object (e.g. a stub in tests): nothing to hook, the reference would count 0 modules
        controller.num_att_layers = 0


class LayerCall:
    """One materialised layer call, from HookAdapter.query to probs_ready: the executor's buffer and what its kernel does to the probabilities."""
    __slots__ = ("buf", "view", "half", "epilogue", "refs", "edit_done", "acc_key")

    def __init__(self, half=False):
        self.buf = self.view = None    # fp16 [rows, nq, ld] and its [:, :, :nk] view, which the controller gets
        self.half = half               # the rows are the conditional half of a [uncond; cond] batch only
        self.epilogue = None           # _lib.ProbsEpilogue for the kernel, or None: the controller does everything itself
        self.refs = []                 # the tensors `epilogue` points into, alive as long as it is
        self.edit_done = False         # the kernel applies this step's edit (cross-attention operator / base prompt's self rows)
        self.acc_key = None            # (key, index): the kernel adds the probabilities to attention_store[key][index]


class HookAdapter:
    """Bridges the executor's C callback (query / probs-ready per Attention module) to a controller object.

    Constraint on what a controller may return for SELF-attention layers: every row of P must still sum to one.  The
    executor folds norm1's beta through attn1.to_v into attn1.to_out's bias at load time (unet.pack_state_dict: P (V + 1 w^T)
    = P V + 1 w^T only when P 1 = 1), so an edit that rescales or un-normalises self-attention rows would see the reference's
    P (V + W_v beta) replaced by P V + W_o W_v beta.  Every shipped controller satisfies it (self-attention edits copy whole
    softmax rows, utils/p2p.py:183-188; Reweight only touches cross-attention, whose V carries no LayerNorm).  Cross-attention
    probabilities are unconstrained."""

    def __init__(self, controller, cond_only: bool, dev, batch: int = 0):
        self.c = controller
        self.cond_only = cond_only
        self.dev = dev
        self.native = self._trusts_needs_probs(controller)
        # arena sizing hint for the executor (icd_unet_workspace_bytes_ex): 1 = the shipped controllers' rule, 2 = any layer
        self.probs_mode = 1 if self.native else 2
        self.call = None                           # the LayerCall in flight, from query to probs_ready
        # for exactly the shipped classes what they do to P - accumulate into the store, copy the base prompt's self-attention rows, the
        # cross-attention edit operator - rides in the probability kernel's epilogue (module docstring)
        self.fuse = (self.native and type(controller) in (AttentionStore, AttentionReplace, AttentionRefine, AttentionReweight, ControllerBatch)
                     and getattr(controller, "fused_epilogue", True) and not LOW_RESOURCE and str(dev).startswith("cuda"))
        # a controller with the reference's __call__ touches the second half of a [uncond; cond] batch only (utils/p2p.py:153-155).  The
        # executor then writes P for those samples alone and runs the unconditional half through the fused kernel (hook return 2): half
        # the probabilities written, read back by P.V and held by the caching allocator
        self.half_ok = (self.native and not cond_only and not LOW_RESOURCE and isinstance(controller, AttentionControl)
                        and type(controller).__call__ is AttentionControl.__call__ and batch > 0 and batch % 2 == 0
                        and getattr(controller, "cond_rows_only", True) and str(dev).startswith("cuda"))
        self.batch = batch                         # samples of the UNet batch ([uncond; cond] when not cond_only); 0 = unknown

    @property
    def half(self):                                # of the layer call in flight, as `epilogue`
        return self.call is not None and self.call.half

    @property
    def epilogue(self):
        return None if self.call is None else self.call.epilogue

    @staticmethod
    def _trusts_needs_probs(c):
        """`needs_probs` may only short-cut a layer when it describes the `forward` that will actually run: the shipped
        forwards (this module), or a subclass that overrides `forward` AND states its own `needs_probs` at or below it in
        the MRO.  A reference-style subclass that only overrides `forward` gets every layer, as utils/p2p.py:336 gives it."""
        if isinstance(c, EmptyControl):
            return True
        if not isinstance(c, AttentionControl):
            return False
        mro = type(c).__mro__
        fwd_owner = next(k for k in mro if "forward" in k.__dict__)
        np_owner = next(k for k in mro if "needs_probs" in k.__dict__)
        if fwd_owner.__module__ == __name__:
            return True
        return mro.index(np_owner) <= mro.index(fwd_owner)

    def query(self, layer, is_cross, place, bh, nq, nk, ld):
        c = self.c
        if self.native and not c.needs_probs(is_cross, nq, place):
            if isinstance(c, AttentionControl):
                c.tick()
            return None
        # a FRESH buffer per layer call: AttentionStore keeps views of it alive across steps (utils/p2p.py:148,153-157)
        half = self.half_ok and bh % 2 == 0
        rows = bh // 2 if half else bh
        call = self.plan(is_cross, place, rows, nq, nk, ld, half) if self.fuse else LayerCall(half)
        call.buf = torch.empty((rows, nq, ld), dtype=torch.float16, device=self.dev)
        call.view = call.buf[:, :, :nk]
        self.call = call
        return call.buf

    def plan(self, is_cross, place, bh, nq, nk, ld, half=False):
        """The LayerCall of a layer whose buffer holds `bh` = samples x heads rows, without its buffer: which of the controller's operations
        on P the probability kernel performs itself (icd_probs_epilogue).  Nothing is launched or allocated."""
        from . import _lib, ops
        c = self.c
        call = LayerCall(half)
        first = 0 if (self.cond_only or half) else bh // 2
        rows = bh - first
        epi = _lib.ProbsEpilogue()
        epi.first_cond_row = first
        if c.layout is not None:
            # operators [group][edit], each group's self rows from its own base.  The kernel indexes them by SAMPLE (prompt jp of its group,
            # operator jp - 1), while the controller - like the reference (utils/p2p.py:192-194) - groups the rows by heads = rows / P: the
            # two agree only when the conditional samples of this call are exactly the controller's prompts.  Anything else (more latents
            # than prompts, an unknown batch) keeps the separate passes.
            G, P = c.layout
            cond = (self.batch if self.cond_only else self.batch // 2) if self.batch > 0 else 0
            if rows % (G * P) != 0 or P < 2 or cond != G * P:
                return call
            epi.edit_count, epi.group_count = P - 1, G
            if is_cross:
                if not ops.p2p_cross_edit_geometry(nk, ld):
                    return call                      # the torch / icd_p2p_cross_edit_groups path handles it (and then the store add must follow it)
                At, Dp = c.cross_edit_operator(c.cur_step, self.dev)
                epi.edit_At, epi.edit_D = At.data_ptr(), Dp.data_ptr()
                call.refs += [At, Dp]
                call.edit_done = True
            else:                                    # (materialised self-attention layers are the <= 32^2-query ones: always replaced)
                win = c.self_window(c.cur_step)
                if win is None:                      # the groups disagree about their self-replace windows: the separate passes
                    return call
                if win:
                    epi.self_from_base = 1
                    call.edit_done = True
        if nq <= c.STORE_MAX_QUERIES:
            key = f"{place}_{'cross' if is_cross else 'self'}"
            target = c.store_target(key, (rows, nq, nk), ld)
            if target is not None:
                epi.acc = target[1].data_ptr()
                call.refs.append(target[1])
                call.acc_key = (key, target[0])
        if call.edit_done or call.acc_key:
            call.epilogue = epi
        return call

    def probs_ready(self, layer, is_cross, place):
        call, self.call = self.call, None
        c = self.c
        fused = call.epilogue is not None
        if fused:                                    # tell the controller what the kernel has done to this layer's P
            c.kernel_did(call.edit_done, call.acc_key)
        try:
            if (self.cond_only or call.half) and isinstance(c, AttentionControl):
                c.call_cond_only(call.view, is_cross, place)
                return
            out = c(call.view, is_cross, place)
            if out is not None and out is not call.view:
                call.view.copy_(out)
        finally:
            if fused:
                c.kernel_did(False)


# ------------------------------------------------------------------------------------------- word / schedule helpers
def get_word_inds(text: str, word_place, tokenizer):
    """Token positions (1-based, after BOS) of a word given by value or by index (utils/p2p.py:422-440): one
    implementation, shared with the aligner."""
    return seq_aligner.get_word_inds(text, word_place, tokenizer)


def _step_gate(bounds, n_rows):
    """0/1 column over the n_rows = num_steps + 1 schedule rows: 1 on [int(lo * n_rows), int(hi * n_rows))."""
    lo, hi = (0.0, bounds) if type(bounds) is float else bounds
    rows = torch.arange(n_rows)
    return ((rows >= int(lo * n_rows)) & (rows < int(hi * n_rows))).float()


def update_alpha_time_word(alpha, bounds, prompt_ind: int, word_inds: Optional[torch.Tensor] = None):
    """Set alpha[:, prompt_ind, word_inds] to the step gate of `bounds` (utils/p2p.py:388-399); all words when None."""
    gate = _step_gate(bounds, alpha.shape[0])
    cols = slice(None) if word_inds is None else torch.as_tensor(np.asarray(word_inds), dtype=torch.int64)
    alpha[:, prompt_ind, cols] = gate[:, None]
    return alpha


def get_time_words_attention_alpha(prompts, num_steps, cross_replace_steps, tokenizer, max_num_words=77):
    """[num_steps+1, n_edits, 1, 1, 77] step x word gate of the cross-attention injection (utils/p2p.py:402-420): the
    "default_" window for every token, overridden per word where a word-specific window is given."""
    windows = dict(cross_replace_steps) if type(cross_replace_steps) is dict else {"default_": cross_replace_steps}
    if type(cross_replace_steps) is dict:
        cross_replace_steps.setdefault("default_", (0., 1.))          # the reference adds the key to the caller's dict
    windows.setdefault("default_", (0., 1.))
    n_edits, rows = len(prompts) - 1, num_steps + 1
    alpha = _step_gate(windows["default_"], rows)[:, None, None].repeat(1, n_edits, max_num_words)
    for word, bounds in windows.items():
        if word == "default_":
            continue
        gate = _step_gate(bounds, rows)
        for e in range(n_edits):
            cols = get_word_inds(prompts[e + 1], word, tokenizer)
            if len(cols) > 0:
                alpha[:, e, torch.as_tensor(cols, dtype=torch.int64)] = gate[:, None]
    return alpha.reshape(rows, n_edits, 1, 1, max_num_words)


def get_equalizer(text: str, word_select, values):
    """[1, 77] per-token scale: `values[k]` on the tokens of word `word_select[k]`, 1 elsewhere (utils/p2p.py:443-453)."""
    if type(word_select) is int or type(word_select) is str:
        word_select = (word_select,)
    eq = torch.ones(1, 77)
    for word, val in zip(word_select, values):
        eq[:, get_word_inds(text, word, tokenizer)] = val
    return eq
