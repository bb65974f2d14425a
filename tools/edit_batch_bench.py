#!/usr/bin/env python3
"""Batched editing throughput: G independent image edits (one [source, edit] pair each) in one UNet batch.

    python tools/edit_batch_bench.py [--pairs 1,2,4,8,16] [--reps 3] [--inflight N]

Workload (the reference's editing driver with its shipped settings, launch_editing_iCD_sd1.5.sh): full-size SD1.5 on synthetic
weights, 64 x 64 latents; per image a 4-step consistency inversion (w = 0, one seed per image), then a 4-step reverse edit at gs 19
with dynamic guidance (tau 0.8), w-embedding 512, a Replace controller (cross 0.3, self 0.6) with LocalBlend and a Reweight amplify
of 4.  With the dead unconditional half eliminated one pair is a UNet batch of 2; G pairs run as G prompt groups
(p2p.ControllerBatch, generation.runner's grouping) in one batch of 2G.  Per G: edited images/s, inversion and edit ms (events, a
synchronise per timed window, one warm-up first), then the per-family kernel table of one edit pass at the largest G.
--inflight N adds G = 1 with N executor replicas in flight (inflight.InFlight), the alternative, in the same process.
"""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", default="1,2,4,8,16")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--inflight", type=int, default=0)
a = ap.parse_args()

from invertible_cd_amd import _lib, build, generation, p2p, synthetic, unet
from invertible_cd_amd.inflight import InFlight
from invertible_cd_amd.pipelines import StableDiffusionPipeline
from invertible_cd_amd.schedulers import DDIMScheduler
from invertible_cd_amd.unet_config import SD15

dev = "cuda"
P = 2
p2p.tokenizer = synthetic.SyntheticTokenizer()
p2p.NUM_DDIM_STEPS = 4
p2p.device = dev
sd = synthetic.synthetic_state_dict(SD15, seed=0, device=dev, dtype=torch.float16)
net0 = unet.UNet2DConditionModel(SD15, sd)
del sd
PAIR = ["a cat sitting on a bench", "a dog sitting on a bench"]


def make_solver(net):
    model = StableDiffusionPipeline(net, DDIMScheduler.sd15(), tokenizer=synthetic.SyntheticTokenizer(), device=dev, dtype=torch.float16)
    solver = generation.Generator(model, 50, DDIMScheduler.sd15(), forward_cons_model=model, reverse_cons_model=model,
                                  reverse_timesteps=[259, 519, 779, 999], forward_timesteps=[19, 259, 519, 779])
    solver.latent2image = lambda z, return_type="np": np.zeros((1,))
    return model, solver


def controller():
    return p2p.make_controller(PAIR, True, 0.3, 0.6, blend_words=(("cat",), ("dog",)),
                               equilizer_params={"words": ("dog",), "values": (4.0,)})


class Edit:
    """G pairs: one batched inversion (G latents, G seeds), one batched edit (G prompt groups of P)."""

    def __init__(self, net, G):
        self.model, self.solver = make_solver(net)
        self.G = G
        g = torch.Generator().manual_seed(453645634 + G)
        self.img = torch.randn(G, 4, 64, 64, generator=g).to(dev)
        self.ctx_inv = torch.randn(2 * G, 77, 768, generator=g).to(dev, torch.float16)
        self.ctx_edit = torch.randn(2 * G * P, 77, 768, generator=g).to(dev, torch.float16)

    def inversion(self):
        self.solver.context = self.ctx_inv
        return self.solver.cons_inversion(self.img, guidance_scale=0.0, w_embed_dim=512, seed=list(range(self.G)))[1][0]

    def edit(self, inv):
        ctrl = p2p.ControllerBatch([controller() for _ in range(self.G)])
        p2p.register_attention_control(self.model, ctrl)
        self.solver.context = self.ctx_edit
        start = inv[:, None].expand(self.G, P, *inv.shape[1:]).reshape(self.G * P, *inv.shape[1:])
        self.solver.prompt_groups = (self.G, P)
        try:
            return self.solver.cons_generation(start, guidance_scale=19.0, w_embed_dim=512, dynamic_guidance=True, tau1=0.8, tau2=0.8,
                                               controller=ctrl)[-1]
        finally:
            self.solver.prompt_groups = None
            p2p.register_attention_control(self.model, None)

    def both(self):
        return self.edit(self.inversion())


def timed(fn, reps):
    fn()                                                             # warm-up (plans, arenas, cached operators)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        r = fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps, r


print(f"# tools/edit_batch_bench.py on {torch.cuda.get_device_name(0)}, kernels_sha {build.source_sha()}, reps {a.reps}")
print("# per G: G [source, edit] pairs; inversion = one batched 4-step consistency inversion of G images, edit = one batched 4-step "
      "reverse edit of G prompt groups (UNet batch 2G, unconditional half eliminated)")
pairs = [int(x) for x in a.pairs.split(",")]
base = None
for G in pairs:
    e = Edit(net0, G)
    t_inv, inv = timed(e.inversion, a.reps)
    t_edit, _ = timed(lambda: e.edit(inv), a.reps)
    ips = G / ((t_inv + t_edit) / 1e3)
    base = base or ips
    print(f"G={G:3d} unet_batch={2 * G:3d}  inversion {t_inv:8.1f} ms  edit {t_edit:8.1f} ms  {ips:7.2f} edited images/s  "
          f"({ips / base:.2f} x G = {pairs[0]})")
    del e, inv
    torch.cuda.empty_cache()

if a.inflight > 1:
    nets = [net0] + [net0.replica() for _ in range(a.inflight - 1)]
    edits = [Edit(n, 1) for n in nets]
    flight = InFlight([e.both for e in edits], torch.device("cuda", torch.cuda.current_device()))
    n_pass = a.inflight * a.reps
    ms, _ = timed(lambda: flight.run(n_pass), 1)
    print(f"G=  1 in_flight={a.inflight}  {n_pass} pairs (inversion + edit each) in {ms:8.1f} ms  {n_pass / (ms / 1e3):7.2f} edited images/s "
          f"({n_pass / (ms / 1e3) / base:.2f} x G = {pairs[0]})")
    del flight, edits, nets

G = pairs[-1]
e = Edit(net0, G)
inv = e.inversion()
e.edit(inv)
torch.cuda.synchronize()
_lib.profile_enable(True)
e.edit(inv)
torch.cuda.synchronize()
print(f"# per-family kernel table of one edit pass at G = {G}")
for k, v in _lib.profile_read().items():
    if v["launches"]:
        print(f"   {k:12s} {v['launches']:6d} launches {v['ms']:9.3f} ms")
_lib.profile_enable(False)
