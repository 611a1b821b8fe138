#!/usr/bin/env python3
"""Measurements around iadr1_sample_logp (profiles/EXPERIMENTS.md "Whole-vocabulary sampling and rollout log-probs"):
  sampler   the two sampler launches on the decode shape (64 x 151936 fp32, rotating buffers), HIP events, us per call: the old entry point, the new one with
            top-k 50 + log-probs, and the whole vocabulary (top_k = 0) + log-probs; then iadr1_sample_ex on the same inputs, neutral and with penalty / min_p
  decode    ms per decode step of the 3B rollout (8 prompts x G = 8, HIP events around the graph replays) with return_logps off / on / top_k = 0
  metrics   rollout/logp_abs_diff_mean|max and rollout/kl of one SC-GRPO step at 3B shapes (8 x 8 x 256 tokens), for the decode weights given by --decode_weights
Usage: python tools/rollout_logps_probe.py sampler | decode [--layers N] | metrics [--layers N] [--decode_weights fp8]"""
import argparse
import dataclasses
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import iadr1_amd  # noqa: E402,F401
from iadr1_amd import ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("what", choices=["sampler", "decode", "metrics"])
ap.add_argument("--layers", type=int, default=0)
ap.add_argument("--steps", type=int, default=255)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--decode_weights", default="bf16", choices=["bf16", "fp8"])
a = ap.parse_args()
dev = torch.device("cuda", 0)


def timed(fn, n=120):
    for i in range(12):
        fn(i)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(n):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


if a.what == "sampler":
    torch.manual_seed(0)
    lg = [torch.randn(64, 151936, device=dev) * 3 for _ in range(6)]
    out = torch.zeros(64, dtype=torch.int64, device=dev)
    lp = torch.zeros(64, 256, device=dev)
    for rep in range(a.reps):
        old = timed(lambda i: ops.sample(lg[i % 6], 0.9, 50, 0.9, 1234, i, out=out))
        new = timed(lambda i: ops.sample_logp(lg[i % 6], 0.9, 50, 0.9, 1234, i % 256, out=out, logp_out=lp))
        wv = timed(lambda i: ops.sample_logp(lg[i % 6], 0.9, 0, 1.0, 1234, i % 256, out=out, logp_out=lp))
        print(f"sampler, us per call (stage 1 + stage 2): sample_topk_topp {old:.1f} | sample_logp top-k 50 + logp {new:.1f} | sample_logp whole vocabulary + logp {wv:.1f}", flush=True)
        # iadr1_sample_ex on the same inputs (profiles/EXPERIMENTS.md "min_p and repetition_penalty"): a bitmap of 700 seen ids per row, marked further by every call
        if rep == 0:
            seen = torch.zeros(64, (151936 + 31) // 32, dtype=torch.int32, device=dev)
            pr = torch.randint(0, 151936, (64, 700), device=dev)
            seen.view(-1).scatter_(0, (torch.arange(64, device=dev)[:, None] * seen.shape[1] + (pr >> 5)).view(-1), torch.ones(64 * 700, dtype=torch.int32, device=dev))
        ex = lambda k, p, mp, pen: timed(lambda i: ops.sample_ex(lg[i % 6], 0.9, k, p, 1234, i % 256, min_p=mp, repetition_penalty=pen, seen=seen, mark_seen=pen != 1.0, out=out, logp_out=lp))
        print(f"sample_ex, us per call: neutral top-k 50 {ex(50, 0.9, 0.0, 1.0):.1f} | top-k 50 + penalty 1.3 + min_p 0.05 {ex(50, 0.9, 0.05, 1.3):.1f} | whole vocabulary: neutral {ex(0, 1.0, 0.0, 1.0):.1f}, "
              f"penalty 1.3 {ex(0, 1.0, 0.0, 1.3):.1f}, min_p 0.05 {ex(0, 1.0, 0.05, 1.0):.1f}, penalty 1.3 + min_p 0.05 {ex(0, 1.0, 0.05, 1.3):.1f}", flush=True)
    sys.exit(0)

import bench  # noqa: E402
from iadr1_amd.params import ParamStore, VLMConfig  # noqa: E402
from iadr1_amd.sc_grpo import GRPOArgs, SCGRPOEngine  # noqa: E402

base = VLMConfig.qwen25vl_3b()
cfg = dataclasses.replace(base, num_hidden_layers=a.layers or base.num_hidden_layers, v_depth=2, v_fullatt=(1,))
pol = ParamStore(cfg, dev, trainable=True, decode_weights=a.decode_weights)
pol.init_random(seed=0)
ref = ParamStore(cfg, dev, trainable=False)
ref.copy_from(pol)
batch = bench.synth_batch(cfg, 8, 512, seed=5)
batch["pixel_values"] = batch["pixel_values"].to(dev)

if a.what == "decode":
    for name, kw in (("default", {}), ("rollout_logps", {"rollout_logps": True}), ("top_k=0 + rollout_logps", {"rollout_logps": True, "top_k": 0, "top_p": 1.0}), ("default again", {})):
        eng = SCGRPOEngine(cfg, pol, ref, GRPOArgs(num_generations=8, max_prompt_length=512, max_completion_length=a.steps + 1, micro_batch_seqs=64, suppress_eos=True, **kw))
        for rep in range(a.reps + 1):
            vis = eng.vision_policy(batch, save=False)
            if eng._rollout is not None:
                eng._rollout.decode_events = []
            eng.rollout(batch, vis=vis)
            torch.cuda.synchronize()
            if rep == 0:
                continue
            ev = eng._rollout.decode_events
            ms, n = sum(e0.elapsed_time(e1) for e0, e1, _, _ in ev), sum(k for _, _, k, _ in ev)
            print(f"decode step [{name}] {ms / n:.4f} ms ({n} steps, layers {cfg.num_hidden_layers})", flush=True)
        del eng
    sys.exit(0)

eng = SCGRPOEngine(cfg, pol, ref, GRPOArgs(num_generations=8, max_prompt_length=512, max_completion_length=256, micro_batch_seqs=64, suppress_eos=True, rollout_logps=True))
reward = lambda comp: np.stack([(np.asarray(comp)[:, 0] % 5).astype(np.float32), (np.asarray(comp)[:, 1] % 3).astype(np.float32)], 1)
m = eng.step(batch, reward, do_optimizer_step=False)
print(f"rollout metrics, 3B shapes (8 x 8 x 256 tokens, layers {cfg.num_hidden_layers}), decode weights {a.decode_weights}, traced {eng.last_step_traced}, co-scheduled {eng.last_step_shadowed}: "
      + ", ".join(f"{k} {v:.4e}" for k, v in m.items() if k.startswith("rollout/")), flush=True)
