#!/usr/bin/env python3
"""What the objective options cost or save (profiles/EXPERIMENTS.md "Dr. GRPO / BNPO loss types, truncation mask and beta = 0"): ms per SCGRPOTrainer.training_step
and peak reserved device memory at the 3B headline shape (8 prompts x G = 8, 512 prompt positions, 256 new tokens, bench.py's synthetic processor and reward
plugins), HIP events around each call, three configurations one after the other in one process, each on a fresh trainer with the same random-init weights:

  default            today's step (beta 0.04, loss_type grpo): the co-scheduled step where it applies
  beta0              beta 0: no frozen reference is built or run, the sequential step
  beta0_drgrpo_mask  beta 0, loss_type dr_grpo, mask_truncated_completions

The first two sample fixed-length completions (EOS suppressed, like bench.py); the third cannot (the option refuses that combination: every row would be masked),
so its rows end where the random-init model samples an EOS, which is almost never: nearly every row is then truncated and masked.  Its line measures what the
path costs, not a realistic mask.  The comparison is between the lines of one run of this probe.
Usage: python tools/objective_probe.py [--reps 5] [--warmup 2] [--layers N]"""
import argparse
import dataclasses
import gc
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
ap.add_argument("--reps", type=int, default=5, help="timed steps per configuration")
ap.add_argument("--warmup", type=int, default=2, help="untimed steps per configuration")
ap.add_argument("--layers", type=int, default=0)
a = ap.parse_args()
dev = torch.device("cuda", 0)
PROMPTS, GROUP, PROMPT_LEN, GEN_LEN = 8, 8, 512, 256

base = VLMConfig.qwen25vl_3b()
cfg = dataclasses.replace(base, num_hidden_layers=a.layers) if a.layers else base
batches = []
for g in range(a.warmup + a.reps):
    b = bench.synth_batch(cfg, PROMPTS, PROMPT_LEN, seed=1234 + g)
    batches.append({"input_ids": torch.from_numpy(b["input_ids"]), "attention_mask": torch.from_numpy(b["attention_mask"]), "pixel_values": b["pixel_values"].to(dev),
                    "image_grid_thw": torch.tensor(b["image_grid_thw"])})
chat = [{"role": "user", "content": [{"type": "image"}, {"type": "text", "text": "Is there any defect in the image?"}]}]
rows = lambda g: [{"prompt": chat, "image": [("synthetic", g, j)], "solution": bench.SOLUTION} for j in range(PROMPTS)]
CONFIGS = [("default", {}, True), ("beta0", {"beta": 0.0}, True),
           ("beta0_drgrpo_mask", {"beta": 0.0, "loss_type": "dr_grpo", "mask_truncated_completions": True}, False)]

shape = f"3B shapes ({PROMPTS} x {GROUP} x {GEN_LEN} tokens, layers {cfg.num_hidden_layers})"
for name, extra, fixed_length in CONFIGS:
    gc.collect()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(dev)
    pol = ParamStore(cfg, dev, trainable=True)
    pol.init_random(seed=0)
    tr = SCGRPOTrainer((cfg, pol), [rewards.accuracy_reward, rewards.consistency_reward],
                       args=GRPOConfig(output_dir="/tmp/iadr1_probe", per_device_train_batch_size=PROMPTS, num_generations=GROUP, max_completion_length=GEN_LEN, micro_batch_seqs=64,
                                       seed=1234, save_steps=0, max_prompt_length=PROMPT_LEN, **extra),
                       train_dataset=None, processing_class=bench.SynthProcessor(batches, bench.CANNED))
    tr.engine.args.suppress_eos = fixed_length
    ms = []
    for g in range(a.warmup + a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        tr.training_step([rows(g)])
        e1.record()
        torch.cuda.synchronize()
        if g >= a.warmup:
            ms.append(e0.elapsed_time(e1))
        if g == a.warmup - 1:
            tr._metrics.clear()
    m = {k: float(np.mean(v)) for k, v in tr._metrics.items()}
    print(f"training_step [{name}] {shape}: median {np.median(ms):.1f} ms, mean {np.mean(ms):.1f}, min {min(ms):.1f}, max {max(ms):.1f} ({len(ms)} steps after {a.warmup} untimed); "
          f"peak reserved {torch.cuda.max_memory_reserved(dev) / 2**30:.2f} GB; co-scheduled {tr.engine.last_step_shadowed}; completion_length {m.get('completion_length', float('nan')):.1f}"
          + (f", clipped_ratio {m['completions/clipped_ratio']:.3f}" if "completions/clipped_ratio" in m else "") + (f", kl {m['kl']:.3e}" if "kl" in m else ", no kl"), flush=True)
    tr.close()
    del tr, pol
