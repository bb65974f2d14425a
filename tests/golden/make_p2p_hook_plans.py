#!/usr/bin/env python3
"""The hook adapter's plans for a fixed walk of layer calls, and the recording of them (tests/golden/p2p_hook_plans.json).

    python3 -B tests/golden/make_p2p_hook_plans.py --write

cases() is a deterministic list of (name, controller factory, G, P, layout): the shipped controllers and ControllerBatches of them on the
batch layouts the executor runs (cond-only, [uncond; cond] with the conditional half or the whole batch materialised) and on the ones it must
refuse to fuse (unknown batch, one latent too many, twice the prompts).  record() walks each through two steps of WALK the way the executor's
hook does - needs_probs / tick, else the plan of the layer call and then the controller on the probabilities - and notes per layer call
whether the layer was short-cut, the counters afterwards and what HookAdapter.plan put into the probability kernel's epilogue struct.  No
GPU and no built library: on the CPU the controllers take their torch expressions and the plan never carries a store pointer (that half is
pinned by the GPU tests).  tests/test_p2p_hook_plans.py replays it.  The golden file was written once from the adapter as it stood BEFORE
its two planning branches became one and is not to be regenerated: a plan that changes on purpose changes its rows with the reason in the
commit.
"""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))):
    if _p not in sys.path:
        sys.path.insert(0, _p)
from invertible_cd_amd import p2p                                                           # noqa: E402
from stubs import StubTokenizer                                                             # noqa: E402

GOLDEN = os.path.join(HERE, "p2p_hook_plans.json")
FIELDS = ("tick", "cur_step", "cur_att_layer", "members_in_step", "planned", "first_cond_row", "edit_count", "groups", "self_from_base",
          "edit_At", "edit_D")
STEP_FIELDS = ("cur_step", "blend_counters")
HEADS, STEPS, NUM_DDIM_STEPS = 2, 2, 4
BIG, SMALL, MID = 34 * 34, 8 * 8, 4 * 4           # queries above AttentionStore.STORE_MAX_QUERIES, a quarter of the 32 x 32 latent's side, an eighth
# the layer kinds of SD1.5's 32 Attention modules in execution order (tests/test_p2p_batch.py::_sd15_walk), one or two of each
WALK = ([("down", False, BIG), ("down", True, BIG)] + [("down", False, SMALL), ("down", True, SMALL)] * 2 + [("mid", False, MID), ("mid", True, MID)]
        + [("up", False, SMALL), ("up", True, SMALL), ("up", False, BIG), ("up", True, BIG)])
# (tokens, row stride) of a cross-attention layer around the kernel's 80-column rule
CROSS_EDGES = ((77, 80), (80, 80), (77, 88), (77, 96), (77, 84), (77, 77), (81, 88), (96, 96))

PAIR_A = ["a cat sitting on a bench", "a dog sitting on a bench"]
PAIR_B = ["a red car on the road", "a red fast car on the road"]
PAIR_C = ["a bird on a tree", "a crow on a tree"]
TRIPLE_A = ["a cat sitting on a bench", "a dog sitting on a bench", "a fox sitting on a bench"]
TRIPLE_B = ["a cat on a mat", "a cat on a rug", "a cat on a bed"]


def _replace(self_steps=0.25):
    return p2p.make_controller(PAIR_A, True, 0.5, self_steps)


def _refine_reweight_blend(self_steps=0.25):
    return p2p.make_controller(PAIR_B, False, {"default_": 0.8, "fast": (0.0, 0.5)}, self_steps, blend_words=(("car",), ("car",)),
                               equilizer_params={"words": ("fast",), "values": (2.0,)})


def _reweight_blend(self_steps=0.25):
    return p2p.make_controller(PAIR_C, True, 0.8, self_steps, blend_words=(("bird",), ("crow",)),
                               equilizer_params={"words": ("crow",), "values": (4.0,)})


CONTROLLERS = (
    # name, factory, prompt groups, prompts per group
    ("store", p2p.AttentionStore, 1, 2),
    ("replace", _replace, 1, 2),
    ("refine_reweight_blend", _refine_reweight_blend, 1, 2),
    ("batch_1x2", lambda: p2p.ControllerBatch([_replace()]), 1, 2),
    ("batch_2x2", lambda: p2p.ControllerBatch([_replace(), _refine_reweight_blend()]), 2, 2),
    ("batch_3x2", lambda: p2p.ControllerBatch([_replace(), _refine_reweight_blend(), _reweight_blend()]), 3, 2),
    ("batch_2x3", lambda: p2p.ControllerBatch([p2p.make_controller(TRIPLE_A, True, 0.5, 0.25, blend_words=(("cat",), ("dog",), ("fox",))),
                                               p2p.make_controller(TRIPLE_B, True, 0.7, 0.25)]), 2, 3),
    ("batch_stores", lambda: p2p.ControllerBatch([p2p.AttentionStore() for _ in range(3)]), 3, 2),
    # self-replace windows [0, 2), [0, 1), [0, 2) of 4 steps: the members agree at step 0 and disagree at step 1
    ("batch_windows_disagree", lambda: p2p.ControllerBatch([_replace(0.5), _refine_reweight_blend(0.25), _reweight_blend(0.6)]), 3, 2),
)


def layouts(n):
    """(name, cond_only, batch, samples materialised, conditional half only, the controller's own batch) for n = G * P conditional samples.
    On a batch that is not the controller's own the walk only ticks the counters: the controller could not group such rows."""
    return (("cond_only", True, n, n, False, True), ("cfg_half", False, 2 * n, n, True, True), ("cfg_whole", False, 2 * n, 2 * n, False, True),
            ("batch_unknown", True, 0, n, False, False), ("one_latent_more", True, n + 1, n + 1, False, False),
            ("cond_only_twice", True, 2 * n, 2 * n, False, False))


def cases():
    return [(f"{cname} | {lname}", make, G, P, lay) for cname, make, G, P in CONTROLLERS for lname, *lay in layouts(G * P)]


def _globals():
    p2p.tokenizer, p2p.device, p2p.NUM_DDIM_STEPS, p2p.LOW_RESOURCE = StubTokenizer(), "cpu", NUM_DDIM_STEPS, False


def plan_fields(adapter, is_cross, place, bh, nq, nk, ld, half):
    epi = adapter.plan(is_cross, place, bh, nq, nk, ld, half=half).epilogue
    if epi is None:
        return [0, 0, 0, 0, 0, 0, 0]
    assert not epi.acc                                   # CPU tensors: the store accumulation is never the kernel's
    return [1, epi.first_cond_row, epi.edit_count, max(epi.group_count, 1), epi.self_from_base, int(bool(epi.edit_At)), int(bool(epi.edit_D))]


def _walk_case(make, G, P, cond_only, batch, samples, half, own):
    c = make()
    c.num_att_layers = len(WALK)
    members = list(getattr(c, "members", ()))
    blends = [b for b in [getattr(m, "local_blend", None) for m in members or [c]] if b is not None]
    adapter = p2p.HookAdapter(c, cond_only, "cpu", batch=batch)
    x = torch.zeros(G * P, 4, 32, 32)
    rows, steps = [], []
    for _ in range(STEPS):
        for place, is_cross, nq in WALK:
            tick = not c.needs_probs(is_cross, nq, place)
            plan = [0, 0, 0, 0, 0, 0, 0]
            if tick:
                c.tick()
            else:
                nk = 77 if is_cross else nq
                bh = samples * HEADS
                plan = plan_fields(adapter, is_cross, place, bh, nq, nk, (nk + 7) // 8 * 8, half)
                if not own:
                    c.tick()
                elif cond_only or half:
                    c.call_cond_only(torch.full((bh, nq, nk), 1.0 / nk), is_cross, place)
                else:
                    c(torch.full((bh, nq, nk), 1.0 / nk), is_cross, place)
            here = (c.cur_step, c.cur_att_layer)
            plan = [int(tick), *here, int(all((m.cur_step, m.cur_att_layer) == here for m in members))] + plan
            rows.append(plan)
        if own:
            x = c.step_callback(x)
        steps.append([c.cur_step, [b.counter for b in blends]])
    return rows, steps


def record():
    _globals()
    got = {"fields": list(FIELDS), "step_fields": list(STEP_FIELDS), "walk": [list(w) for w in WALK], "cases": {}, "cross_edges": []}
    for name, make, G, P, lay in cases():
        rows, steps = _walk_case(make, G, P, *lay)
        got["cases"][name] = {"rows": rows, "steps": steps}
    for make, G in ((_replace, 1), (lambda: p2p.ControllerBatch([_replace(), _reweight_blend()]), 2)):
        adapter = p2p.HookAdapter(make(), True, "cpu", batch=2 * G)
        got["cross_edges"].append([plan_fields(adapter, True, "down", 2 * G * HEADS, SMALL, nk, ld, False) for nk, ld in CROSS_EDGES])
    return got


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit(__doc__)
    with open(GOLDEN, "w") as f:
        json.dump(record(), f, separators=(",", ":"))
        f.write("\n")
    print(f"wrote {GOLDEN}")
