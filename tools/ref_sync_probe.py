#!/usr/bin/env python3
"""What GRPOConfig.sync_ref_model costs on the steps that sync (profiles/EXPERIMENTS.md "sync_ref_model"): ms per SCGRPOEngine.optimizer_step at the 3B shapes
with and without the reference mix, HIP events around each call, one process -- ref_model_sync_steps 2, so the two kinds of step alternate in the same run on
the same buffers -- and the mix pass alone (ParamStore.mix_from with and without the distance sums) next to the AdamW launches alone, with the bytes each moves
(6 B per parameter for the mix: two bf16 reads and one write; 22 B for iadr1_adamw_flat: four fp32 reads, four fp32 writes, one bf16 write).
The gradients are zero: none of these passes' time depends on values.
Usage: python tools/ref_sync_probe.py [--reps 20] [--warmup 4] [--layers N] [--alpha 0.6]"""
import argparse
import dataclasses
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import iadr1_amd  # noqa: E402,F401
from iadr1_amd import hip  # noqa: E402
from iadr1_amd.params import ParamStore, VLMConfig  # noqa: E402
from iadr1_amd.sc_grpo import GRPOArgs, SCGRPOEngine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20, help="timed optimizer steps of each kind")
ap.add_argument("--warmup", type=int, default=4, help="untimed optimizer steps")
ap.add_argument("--layers", type=int, default=0)
ap.add_argument("--alpha", type=float, default=0.6)
a = ap.parse_args()
assert torch.cuda.is_available(), "ref_sync_probe needs the GPU: there is no CPU path to time"
dev = torch.device("cuda", 0)
base = VLMConfig.qwen25vl_3b()
cfg = dataclasses.replace(base, num_hidden_layers=a.layers) if a.layers else base
pol, ref = ParamStore(cfg, dev, trainable=True), ParamStore(cfg, dev, trainable=False)
pol.init_random(seed=0)
ref.init_random(seed=1)
eng = SCGRPOEngine(cfg, pol, ref, GRPOArgs(sync_ref_model=True, ref_model_mixup_alpha=a.alpha, ref_model_sync_steps=2, learning_rate=1e-6))
n = pol.n_total


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def line(what, v, nbytes=None):
    rate = f", {nbytes / (np.median(v) * 1e-3) / 1e9:.0f} GB/s at the median" if nbytes else ""
    print(f"{what}: median {np.median(v):.3f} ms, mean {np.mean(v):.3f}, min {min(v):.3f}, max {max(v):.3f} ({len(v)} calls){rate}", flush=True)


ms = {"plain": [], "sync": []}
for k in range(a.warmup + 2 * a.reps):
    t = timed(eng.optimizer_step)
    if k >= a.warmup:
        ms["sync" if eng.opt_step % 2 == 0 else "plain"].append(t)
print(f"3B shapes, layers {cfg.num_hidden_layers}: {n} parameters ({n * 2 / 1e9:.2f} GB of bf16 per copy), alpha {a.alpha:g}, {eng.ref_syncs} syncs in all", flush=True)
line("optimizer_step without a sync", ms["plain"])
line("optimizer_step with the sync ", ms["sync"])
print(f"difference of the medians: {np.median(ms['sync']) - np.median(ms['plain']):.3f} ms per sync step", flush=True)

dist2 = torch.zeros(2, dtype=torch.float32, device=dev)
for _ in range(2):
    ref.mix_from(pol, a.alpha, dist2)
    ref.mix_from(pol, a.alpha)
line("mix_from with the distance sums (2 launches)", [timed(lambda: ref.mix_from(pol, a.alpha, dist2)) for _ in range(a.reps)], 6 * n)
line("mix_from without                 (1 launch)", [timed(lambda: ref.mix_from(pol, a.alpha)) for _ in range(a.reps)], 6 * n)


def adamw():
    for lo, hi, wd in ((0, pol.n_decay, 0.0), (pol.n_decay, n, 0.0)):
        hip.call("adamw_flat", pol.master[lo:hi], pol.m[lo:hi], pol.v[lo:hi], pol.grad[lo:hi], pol.flat[lo:hi], hi - lo, 1e-6, 0.9, 0.999, 1e-8, wd, 1, 1.0, eng.norm2, 1.0)


adamw()
line("the two iadr1_adamw_flat launches alone", [timed(adamw) for _ in range(a.reps)], 22 * n)
