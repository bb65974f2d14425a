"""The launch sequence of AutoencoderKL, pinned without a GPU: a recorder stands in for `vae.ops`, keeps the two host-side weight packers
real, and answers every launch with an empty CPU tensor of the shape and dtype the real operator returns.  Each launch becomes one line:
the op, the shapes and dtypes of its tensor arguments, its geometry scalars, and which of the optional operands are present (weight
contents are not recorded: einsum bits may differ between hosts).  tests/golden/vae_launch_trace.json holds the sequences of the commit
before the fp16 and fp32-fidelity walks were merged into one; the test asserts the whole sequence of every case.

    python tests/test_vae_trace.py          # rewrites the fixture from the checked-out vae.py: only ever from a commit whose launches
                                            # are the ones to keep (a refactor regenerates it at its parent, never from its own code)
"""
import inspect
import json
import os
import sys

import pytest
import torch

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from invertible_cd_amd import ops, vae

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vae_launch_trace.json")
SCALARS = ("B", "H", "W", "stride", "upsample", "pad_hi", "phase", "silu", "out_f32", "cout", "ones_channel", "out_dtype")
PRESENT = ("resid", "resid_carry", "out_carry", "out", "alpha")
F16, F32 = torch.float16, torch.float32


def _e(*shape, dtype=F16):
    return torch.empty(shape, dtype=dtype)


def _conv3x3(a):
    if a["phase"] is not None:
        return a["out"]
    s, up = a["stride"], 2 if a["upsample"] else 1
    return _e(a["B"] * ((a["H"] * up + s - 1) // s) * ((a["W"] * up + s - 1) // s), a["w_packed"].shape[0], dtype=F32 if a["out_f32"] else F16)


def _split3(a):
    return _e(a["x32"].shape[0], 3 * a["x32"].shape[1])


def _flash(a):
    return _e(a["B"] * a["Nq"], a["H"] * a["d"])


RETURNS = {                                  # op -> what it returns, from its bound arguments (defaults applied)
    "groupnorm": lambda a: _e(*a["x"].shape),
    "groupnorm_carry": lambda a: _e(*a["x"].shape),
    "groupnorm_f32_split": _split3,
    "split_cast": _split3,
    "split_cast_guarded": lambda a: (_split3(a), 1.0),
    "pack_nchw": lambda a: _e(a["x_nchw"].shape[0] * a["x_nchw"].shape[2] * a["x_nchw"].shape[3], 8),
    "conv3x3": _conv3x3,
    "gemm": lambda a: _e(a["a"].shape[0], a["w"].shape[0], dtype=F32 if a["out_f32"] else F16),
    "conv_out": lambda a: _e(a["B"], a["cout"], a["H"], a["W"], dtype=a["out_dtype"]),
    "project_vt": lambda a: _e(a["B"], a["w"].shape[0], a["ld_keys"]),
    "attention_fused": _flash,
    "attention_wide": _flash,
    "attention_scores": lambda a: _e(a["B"] * a["H"], a["Nq"], a["ld"], dtype=F32),
    "softmax_rows": lambda a: _e(a["s"].shape[0], a["ld_p"]),
    "attention_apply": lambda a: a["out"],
}


class Recorder:
    """Stands in for `vae.ops`; an operator it does not know is an AttributeError, so a new launch cannot pass unrecorded."""
    pack_conv_weight = staticmethod(ops.pack_conv_weight)
    split_weight = staticmethod(ops.split_weight)

    def __init__(self):
        self.trace = []

    def __getattr__(self, name):
        if name not in RETURNS:
            raise AttributeError(f"the VAE asked for ops.{name}, which the recorder does not know")
        sig = inspect.signature(getattr(ops, name))

        def launch(*args, **kw):
            bound = sig.bind(*args, **kw)
            given = {k for k, v in bound.arguments.items() if v is not None}
            bound.apply_defaults()
            a = bound.arguments
            tensors = [f"{k}:{'x'.join(map(str, v.shape))}:{str(v.dtype)[6:]}" for k, v in a.items() if isinstance(v, torch.Tensor)]
            scalars = [f"{k}={str(a[k]).replace('torch.', '')}" for k in SCALARS if k in a]
            self.trace.append(" ".join([name] + tensors + ["|"] + scalars + ["|"] + [k for k in PRESENT if k in given]))
            return RETURNS[name](a)
        return launch


CFG = vae.SD_VAE.scaled((32, 64, 64, 64))
B, CHUNK = 3, 2                                                  # a ragged last chunk
LATENT, IMAGE = (5, 7), (40, 56)                                 # odd maps at every level; W < 2 is never reached


def _case(kind, dtype, carry=True, phases=True, fused=None, hw=None):
    return dict(kind=kind, dtype=dtype, carry=carry, phases=phases, fused=fused, hw=hw or (LATENT if kind == "decode" else IMAGE))


CASES = {f"decode fp16 carry={c} upsample_phases={p}": _case("decode", F16, carry=c, phases=p) for c in (True, False) for p in (True, False)}
CASES.update({f"decode fp16 fused_attention={f}": _case("decode", F16, fused=f) for f in (None, True, False)})
CASES["decode fp32"] = _case("decode", F32)
CASES["encode fp16"] = _case("encode", F16)
CASES["encode fp16 carry=False"] = _case("encode", F16, carry=False)
CASES["encode fp32"] = _case("encode", F32)
CASES["decode fp16 latent 1x1"] = _case("decode", F16, hw=(1, 1))       # W >= 2 fails at the first upsampler: its 3 x 3 form


def record(case):
    sd = {k: torch.zeros(s) for k, s in CFG.state_dict_shapes().items()}
    rec, real = Recorder(), vae.ops
    vae.ops = rec
    try:
        m = vae.AutoencoderKL(CFG, sd, device="cpu", dtype=case["dtype"], max_chunk=CHUNK, fused_attention=case["fused"])
        m.carry, m.upsample_phases = case["carry"], case["phases"]
        if case["kind"] == "decode":
            m.decode(torch.zeros(B, 4, *case["hw"]))
        else:
            m.encode(torch.zeros(B, 3, *case["hw"]))
    finally:
        vae.ops = real
    return rec.trace


@pytest.mark.parametrize("name", list(CASES))
def test_launch_sequence_is_the_pinned_one(name):
    with open(FIXTURE) as f:
        want = json.load(f)[name]
    got = record(CASES[name])
    assert len(got) == len(want), f"{len(got)} launches, the fixture has {len(want)}"
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"launch {i} differs"


if __name__ == "__main__":
    with open(FIXTURE, "w") as f:
        json.dump({name: record(case) for name, case in CASES.items()}, f, indent=0)
        f.write("\n")
