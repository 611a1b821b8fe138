#!/usr/bin/env python3
"""What a reuse step costs (profiles/EXPERIMENTS.md "Reuse each rollout for num_iterations steps with a clipped GRPO loss"): ms per SCGRPOTrainer.training_step
at the 3B headline shape (8 prompts x G = 8, 512 prompt positions, 256 new tokens, fixed-length completions, bench.py's synthetic processor and reward plugins)
for the step that rolls out and for the steps that reuse its rollout, HIP events around each call, one process; and clip_ratio/region_mean,
policy/ratio_mean and policy/logp_abs_diff_max of the reuse steps at the default learning rate.  With --num_iterations 1 only the generation step exists:
that is today's step, the number to hold the generation step of a reuse run against.
Usage: python tools/num_iterations_probe.py [--num_iterations 2] [--reps 5] [--warmup 2] [--layers N] [--learning_rate LR]"""
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
from iadr1_amd import rewards  # noqa: E402
from iadr1_amd.params import ParamStore, VLMConfig  # noqa: E402
from iadr1_amd.trainer import GRPOConfig, SCGRPOTrainer  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--num_iterations", type=int, default=2)
ap.add_argument("--reps", type=int, default=5, help="timed generations")
ap.add_argument("--warmup", type=int, default=2, help="untimed generations")
ap.add_argument("--layers", type=int, default=0)
ap.add_argument("--learning_rate", type=float, default=None, help="default: GRPOConfig's; 0 leaves the weights alone, so the reuse steps' policy/* then show the distance between "
                "the log-probs a generation step scores (on the rows its decode steps stored) and the ones a full policy forward scores")
a = ap.parse_args()
dev = torch.device("cuda", 0)
PROMPTS, GROUP, PROMPT_LEN, GEN_LEN = 8, 8, 512, 256

base = VLMConfig.qwen25vl_3b()
cfg = dataclasses.replace(base, num_hidden_layers=a.layers) if a.layers else base
pol = ParamStore(cfg, dev, trainable=True)
pol.init_random(seed=0)
batches = []
for g in range(a.warmup + a.reps):
    b = bench.synth_batch(cfg, PROMPTS, PROMPT_LEN, seed=1234 + g)
    batches.append({"input_ids": torch.from_numpy(b["input_ids"]), "attention_mask": torch.from_numpy(b["attention_mask"]), "pixel_values": b["pixel_values"].to(dev),
                    "image_grid_thw": torch.tensor(b["image_grid_thw"])})
chat = [{"role": "user", "content": [{"type": "image"}, {"type": "text", "text": "Is there any defect in the image?"}]}]
rows = lambda g: [{"prompt": chat, "image": [("synthetic", g, j)], "solution": bench.SOLUTION} for j in range(PROMPTS)]
tr = SCGRPOTrainer((cfg, pol), [rewards.accuracy_reward, rewards.consistency_reward],
                   args=GRPOConfig(output_dir="/tmp/iadr1_probe", per_device_train_batch_size=PROMPTS, num_generations=GROUP, max_completion_length=GEN_LEN, micro_batch_seqs=64,
                                   seed=1234, save_steps=0, max_prompt_length=PROMPT_LEN, num_iterations=a.num_iterations,
                                   **({} if a.learning_rate is None else {"learning_rate": a.learning_rate})),
                   train_dataset=None, processing_class=bench.SynthProcessor(batches, bench.CANNED))
tr.engine.args.suppress_eos = True

ms = {"generation": [], "reuse": []}
for g in range(a.warmup + a.reps):
    for it in range(a.num_iterations):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        tr.training_step([rows(g)])
        e1.record()
        torch.cuda.synchronize()
        if g >= a.warmup:
            ms["generation" if it == 0 else "reuse"].append(e0.elapsed_time(e1))
    if g == a.warmup - 1:
        tr._metrics.clear()
shape = f"3B shapes ({PROMPTS} x {GROUP} x {GEN_LEN} tokens, layers {cfg.num_hidden_layers}), num_iterations {a.num_iterations}"
for kind, v in ms.items():
    if v:
        print(f"training_step [{kind}] {shape}: mean {np.mean(v):.1f} ms, median {np.median(v):.1f}, min {min(v):.1f}, max {max(v):.1f} ({len(v)} steps after {a.warmup} untimed generations)", flush=True)
if ms["reuse"]:
    print(f"reuse / generation (medians): {np.median(ms['reuse']) / np.median(ms['generation']):.3f}", flush=True)
    keys = ("clip_ratio/low_mean", "clip_ratio/high_mean", "clip_ratio/region_mean", "policy/ratio_mean", "policy/logp_abs_diff_max")
    print(f"reuse steps at learning rate {tr.args.learning_rate:g}, epsilon {tr.args.epsilon:g}: "
          + ", ".join(f"{k} mean {np.mean(tr._metrics[k]):.4e} max {np.max(tr._metrics[k]):.4e}" for k in keys if k in tr._metrics), flush=True)
