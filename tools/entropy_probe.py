#!/usr/bin/env python3
"""What the rollout's entropy output costs (profiles/EXPERIMENTS.md "Policy entropy from the rollout sampler"):
  decode    ms per decode step of the 3B rollout (8 prompts x G = 8 = 64 sequences, HIP events around the graph replays) without GRPOArgs.rollout_entropy, with it, and
            without it again, in one process on one build.  EOS is suppressed, so all three run the same number of steps; the tokens of the three are compared.
Usage: python tools/entropy_probe.py decode [--layers N] [--steps N] [--reps N]"""
import argparse
import dataclasses
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import iadr1_amd  # noqa: E402,F401
from iadr1_amd.params import ParamStore, VLMConfig  # noqa: E402
from iadr1_amd.sc_grpo import GRPOArgs, SCGRPOEngine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("what", choices=["decode"])
ap.add_argument("--layers", type=int, default=0)
ap.add_argument("--steps", type=int, default=255)
ap.add_argument("--reps", type=int, default=3)
a = ap.parse_args()

dev = torch.device("cuda", 0)
base = VLMConfig.qwen25vl_3b()
cfg = dataclasses.replace(base, num_hidden_layers=a.layers or base.num_hidden_layers, v_depth=2, v_fullatt=(1,))
pol = ParamStore(cfg, dev, trainable=True)
pol.init_random(seed=0)
ref = ParamStore(cfg, dev, trainable=False)
ref.copy_from(pol)
batch = bench.synth_batch(cfg, 8, 512, seed=5)
batch["pixel_values"] = batch["pixel_values"].to(dev)
res, toks_of = {}, {}
for name, kw in (("off", {}), ("entropy", {"rollout_entropy": True}), ("off again", {})):
    eng = SCGRPOEngine(cfg, pol, ref, GRPOArgs(num_generations=8, max_prompt_length=512, max_completion_length=a.steps + 1, micro_batch_seqs=64, suppress_eos=True, **kw))
    for rep in range(a.reps + 1):
        vis = eng.vision_policy(batch, save=False)
        if eng._rollout is not None:
            eng._rollout.decode_events = []
        toks = eng.rollout(batch, vis=vis)
        torch.cuda.synchronize()
        if rep == 0:
            continue
        ev = eng._rollout.decode_events
        ms, n = sum(e0.elapsed_time(e1) for e0, e1, _, _ in ev), sum(k for _, _, k, _ in ev)
        res.setdefault(name, []).append(ms / n)
        ent = eng.last_rollout_entropy
        print(f"decode step [{name}] {ms / n:.4f} ms ({n} steps, layers {cfg.num_hidden_layers}"
              f"{'' if ent is None else f', mean entropy {float(ent.mean()):.4f} of ln V = {np.log(cfg.vocab_size):.4f}'})", flush=True)
    toks_of[name] = np.asarray(toks).copy()
    del eng
assert np.array_equal(toks_of["off"], toks_of["entropy"]) and np.array_equal(toks_of["off"], toks_of["off again"]), "the entropy output changed the tokens"
med = {k: float(np.median(v)) for k, v in res.items()}
print(f"decode step, median of {a.reps}: off {med['off']:.4f} ms, entropy {med['entropy']:.4f} ms, ratio {med['entropy'] / med['off']:.4f} (off again {med['off again']:.4f} ms); tokens equal",
      flush=True)
