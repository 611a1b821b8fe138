#!/usr/bin/env python3
"""Measurements around regex-guided decoding (profiles/EXPERIMENTS.md "Regex-guided decoding"):
  build     host only: guide.compile_regex + guide.TokenGuide.build for the recipe's pattern over a synthetic 151936-token byte-level vocabulary (all 256 single
            bytes, the recipe's tag words, random 2..12-byte pieces of printable text; the ids from 151643 on unemittable, as Qwen2.5's specials and padding are)
  decode    ms per decode step of the 3B rollout (8 prompts x G = 8 = 64 sequences, HIP events around the graph replays), without the guide and with it, in one
            process on one build; EOS is live in both (the guide decides where it goes), so the step counts differ and the figure is per step
Usage: python tools/guided_probe.py build | decode [--layers N] [--steps N] [--reps N]"""
import argparse
import dataclasses
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import iadr1_amd  # noqa: E402,F401
from iadr1_amd import guide  # noqa: E402

PATTERN = r"<think>[\s\S]*?</think><location>[\s\S]*?</location><type>[\s\S]*?</type><answer>(Yes|No)</answer>"
V, N_REGULAR, EOS = 151936, 151643, 151645


def synthetic_vocab():
    rng = np.random.default_rng(0)
    toks = [bytes([b]) for b in range(256)]
    toks += [w.encode() for w in ("<think>", "</think>", "<location>", "</location>", "<type>", "</type>", "<answer>", "</answer>", "think", "location", "type", "answer", "</", "><", ">",
                                  "Yes", "No", " Yes", " No", "es", "Ye")]
    alphabet = np.frombuffer(b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789 .,;:!?<>/()-_'\"\n", dtype=np.uint8)
    have = set(toks)
    while len(toks) < N_REGULAR:
        t = bytes(rng.choice(alphabet, size=int(rng.integers(2, 13))))
        if t not in have:
            have.add(t)
            toks.append(t)
    return toks + [None] * (V - N_REGULAR)


def build_guide(verbose=True):
    t0 = time.perf_counter()
    dfa = guide.compile_regex(PATTERN)
    t1 = time.perf_counter()
    vocab = synthetic_vocab()
    t2 = time.perf_counter()
    g = guide.TokenGuide.build(dfa, vocab, EOS, V)
    t3 = time.perf_counter()
    if verbose:
        print(f"guide build: regex -> {dfa.n} byte-level states in {t1 - t0:.2f} s; tables for V = {V} ({sum(b is not None for b in vocab)} emittable tokens, longest "
              f"{max(len(b) for b in vocab if b)} bytes): {g.S} states, allow {g.allow.nbytes / 1e6:.2f} MB + trans {g.trans.nbytes / 1e6:.2f} MB, in {t3 - t2:.2f} s", flush=True)
    return g


ap = argparse.ArgumentParser()
ap.add_argument("what", choices=["build", "decode"])
ap.add_argument("--layers", type=int, default=0)
ap.add_argument("--steps", type=int, default=255)
ap.add_argument("--reps", type=int, default=3)
a = ap.parse_args()

if a.what == "build":
    for _ in range(a.reps):
        build_guide()
    sys.exit(0)

import torch  # noqa: E402

import bench  # noqa: E402
from iadr1_amd.params import ParamStore, VLMConfig  # noqa: E402
from iadr1_amd.sc_grpo import GRPOArgs, SCGRPOEngine  # noqa: E402

dev = torch.device("cuda", 0)
g = build_guide()
base = VLMConfig.qwen25vl_3b()
cfg = dataclasses.replace(base, num_hidden_layers=a.layers or base.num_hidden_layers, v_depth=2, v_fullatt=(1,))
assert cfg.vocab_size == V and cfg.eos_token_id == EOS, (cfg.vocab_size, cfg.eos_token_id)
pol = ParamStore(cfg, dev, trainable=True)
pol.init_random(seed=0)
ref = ParamStore(cfg, dev, trainable=False)
ref.copy_from(pol)
batch = bench.synth_batch(cfg, 8, 512, seed=5)
batch["pixel_values"] = batch["pixel_values"].to(dev)
res = {}
for name, kw in (("no guide", {}), ("guide", {"guide": g}), ("no guide again", {})):
    eng = SCGRPOEngine(cfg, pol, ref, GRPOArgs(num_generations=8, max_prompt_length=512, max_completion_length=a.steps + 1, micro_batch_seqs=64, **kw))
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
        print(f"decode step [{name}] {ms / n:.4f} ms ({n} steps, layers {cfg.num_hidden_layers}, rows that ended {int((toks == cfg.eos_token_id).any(1).sum())}/64)", flush=True)
    del eng
med = {k: float(np.median(v)) for k, v in res.items()}
print(f"decode step, median of {a.reps}: no guide {med['no guide']:.4f} ms, guide {med['guide']:.4f} ms, ratio {med['guide'] / med['no guide']:.4f} (no guide again {med['no guide again']:.4f} ms)", flush=True)
