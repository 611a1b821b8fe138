"""The rollout returns the log-probs of what it sampled (Rollout.generate(return_logps=True), GRPOArgs.rollout_logps), samples the whole vocabulary for
top_k <= 0, and the evaluation harness samples with --temperature.  GPU only."""
import dataclasses
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fixture_util as fx  # noqa: E402
import iadr1_amd  # noqa: E402,F401
from iadr1_amd.params import ParamStore, VLMConfig  # noqa: E402
from iadr1_amd.sc_grpo import GRPOArgs, SCGRPOEngine  # noqa: E402

DEV = "cuda"
CFG = VLMConfig.from_dict(fx.TINY)
_SEQUENTIAL = {}      # rollout log-probs of the sequential 3B-width step, compared by the co-scheduled case that follows it


def stores(cfg=CFG, kind=None):
    w = fx.make_weights(fx.TINY, 0)
    pol, ref = ParamStore(cfg, DEV, trainable=True, decode_weights=kind), ParamStore(cfg, DEV, trainable=False)
    pol.load_named(w)
    ref.load_named(w)
    return pol, ref


def tiny_batch():
    """The batch of test_sampled_rollout_is_reproducible_and_in_vocab."""
    grids = [(1, 16, 12), (1, 8, 8)]
    rows = [fx.synth_prompt(gr, n, fx.TINY, 77 + i) for i, (gr, n) in enumerate(zip(grids, [5, 17]))]
    ids, mask = fx.left_pad(rows, fx.TINY["pad_token_id"])
    return {"input_ids": ids, "attention_mask": mask, "pixel_values": fx.synth_pixel_values(grids, fx.TINY, seed=77), "image_grid_thw": grids}


def reward_fn(comp):
    return np.stack([(np.asarray(comp)[:, 0] % 5).astype(np.float32), (np.asarray(comp)[:, 1] % 3).astype(np.float32)], 1)


def roll(cfg=CFG, **kw):
    pol, ref = stores(cfg)
    eng = SCGRPOEngine(cfg, pol, ref, GRPOArgs(num_generations=4, max_prompt_length=4096, max_completion_length=16, seed=5, **kw))
    toks = eng.rollout(tiny_batch())
    return toks, (None if eng.last_rollout_logps is None else eng.last_rollout_logps.cpu().numpy())


def test_rollout_returns_logps_without_changing_the_tokens():
    """(6) tokens bit-equal to the call without return_logps; graph and eager log-probs bit-equal; two runs equal; every live position holds a log-prob (< 0);
    zeros after a sequence's first EOS; top_k = 0, top_p = 1.0 reproducible and in vocabulary."""
    t0, none = roll()
    assert none is None
    t1, lp1 = roll(rollout_logps=True)
    t2, lp2 = roll(rollout_logps=True)
    t3, lp3 = roll(rollout_logps=True, use_hip_graph=False)
    assert np.array_equal(t0, t1) and np.array_equal(t1, t2) and np.array_equal(t1, t3)
    assert lp1.shape == t1.shape and np.array_equal(lp1, lp2) and np.array_equal(lp1, lp3)
    live = np.ones_like(t1, dtype=bool)
    for r in range(t1.shape[0]):
        e = np.flatnonzero(t1[r] == CFG.eos_token_id)
        if e.size:
            live[r, e[0] + 1:] = False
    assert (lp1[live] < 0).all() and np.isfinite(lp1).all() and (lp1[~live] == 0).all()
    # EOS: declare a token the sampler draws in the middle of some rows to be EOS; sampling is a pure function of (seed, step, row, logits)
    best = max(np.unique(t1[:, 2:12]), key=lambda tok: sum(tok in t1[r, 2:12] and tok not in t1[r, :2] for r in range(t1.shape[0])))
    cfg2 = dataclasses.replace(CFG, eos_token_id=int(best))
    te, lpe = roll(cfg2, rollout_logps=True)
    ended = 0
    for r in range(te.shape[0]):
        e = np.flatnonzero(te[r] == best)
        n = e[0] + 1 if e.size else te.shape[1]
        ended += bool(e.size) and n < te.shape[1]
        assert np.array_equal(te[r, :n], t1[r, :n]) and np.array_equal(lpe[r, :n], lp1[r, :n]) and (lpe[r, :n] < 0).all() and (lpe[r, n:] == 0).all(), r
    assert ended > 0
    a, la = roll(top_k=0, top_p=1.0, rollout_logps=True)
    b, lb = roll(top_k=0, top_p=1.0, rollout_logps=True)
    c, _ = roll(top_k=0, top_p=1.0)
    assert np.array_equal(a, b) and np.array_equal(la, lb) and np.array_equal(a, c)
    assert a.min() >= 0 and a.max() < fx.TINY["text"]["vocab_size"] and not np.array_equal(a, t1)


def _step(eng, batch):
    out = eng.step(batch, reward_fn, do_optimizer_step=False, return_outputs=True)
    torch.cuda.synchronize()
    return out


def test_engine_step_metrics_leave_the_step_unchanged():
    """(8, TINY part) SCGRPOEngine.step with rollout_logps=True: loss, completion ids, logps, kl and the gradients bit-equal to the step with the flag off; the three
    metrics present and finite, absent with the flag off."""
    batch = tiny_batch()
    res = {}
    for flag in (False, True):
        pol, ref = stores()
        eng = SCGRPOEngine(CFG, pol, ref, GRPOArgs(num_generations=4, max_prompt_length=4096, max_completion_length=16, seed=5, rollout_logps=flag))
        out = _step(eng, batch)
        res[flag] = (out, pol.grad.clone())
    (o0, g0), (o1, g1) = res[False], res[True]
    assert o0["metrics"]["loss"] == o1["metrics"]["loss"] and o0["metrics"]["kl"] == o1["metrics"]["kl"]
    assert np.array_equal(o0["completion_ids"], o1["completion_ids"]) and torch.equal(o0["logps"], o1["logps"]) and torch.equal(o0["kl"], o1["kl"]) and torch.equal(g0, g1)
    keys = ("rollout/logp_abs_diff_mean", "rollout/logp_abs_diff_max", "rollout/kl")
    assert not any(k in o0["metrics"] for k in keys) and "rollout_logps" not in o0 and set(o0["metrics"]) | set(keys) == set(o1["metrics"])
    m = o1["metrics"]
    print("[rollout logps] TINY bf16:", {k: m[k] for k in keys})
    assert all(np.isfinite(m[k]) for k in keys) and m["rollout/logp_abs_diff_max"] >= m["rollout/logp_abs_diff_mean"] >= 0 and m["rollout/kl"] >= 0
    assert tuple(o1["rollout_logps"].shape) == tuple(o1["logps"].shape)


def test_fp8_decode_weights_show_in_the_metric():
    """(9) The same step on ParamStore(decode_weights="fp8"): logp_abs_diff_mean strictly larger than with bf16 weights on the same batch and seed."""
    batch = tiny_batch()
    got = {}
    for kind in ("bf16", "fp8"):
        pol, ref = stores(kind=kind)
        eng = SCGRPOEngine(CFG, pol, ref, GRPOArgs(num_generations=4, max_prompt_length=4096, max_completion_length=16, seed=5, rollout_logps=True))
        got[kind] = _step(eng, batch)["metrics"]
        print(f"[rollout logps] TINY {kind}:", {k: v for k, v in got[kind].items() if k.startswith("rollout/")})
    assert got["fp8"]["rollout/logp_abs_diff_mean"] > got["bf16"]["rollout/logp_abs_diff_mean"]


@pytest.mark.parametrize("overlap_cus", ["0", "64"])
def test_rollout_logps_against_float64_from_the_stored_final_norm_rows(monkeypatch, overlap_cus):
    """(7, and the bound of 8) An engine step whose decode steps fill the training arena (reuse_decode): the returned log-probs against a float64 recomputation on the
    CPU from the final-norm rows those steps stored (`hf`, bf16) and the lm_head weights; column 0 from the prompt's last `hf` row of the prefill.
    |d lse| <= max |d logit|, so |d logp| <= 2 x the bound test_gemm_skinny holds the skinny GEMM's fp32 logits to (rtol 1e-4, atol 1e-3 * sqrt(K) * 0.1, K = hidden
    size).  rollout/logp_abs_diff_max (sampled vs the loss's scored log-probs, which read the same rows through the fused lm_head) within twice that.
    Shapes: the hand-over needs the persistent fused decode kernels (hidden a multiple of 1024), which the TINY fixture (hidden 256) does not take -- there the
    loss scores rows of its own forward, not the decode steps' -- so this runs the 2-layer model at Qwen2.5-VL-3B widths of test_api_step_with_rollout_handover,
    sequential ("0") and co-scheduled ("64": skipped with the reason on a box without a clean stream pair, as there); both give bit-equal rollout log-probs."""
    import test_hip_model as thm
    monkeypatch.setenv("IADR1_OVERLAP_CUS", overlap_cus)
    # a rollout sized for fewer CUs splits the o projection's K differently (fp32 partial sums in another order -> other logits): the same split both ways, as in
    # test_chunked_reference_pass_is_bit_equal_to_the_one_shot_pass
    monkeypatch.setenv("IADR1_DECODE_KS", "1,8")
    cfg = dataclasses.replace(VLMConfig.qwen25vl_3b(), num_hidden_layers=2, v_depth=2, v_fullatt=(1,))
    ref = ParamStore(cfg, DEV, trainable=False)
    ref.init_random(seed=0)
    pol = ParamStore(cfg, DEV, trainable=True)
    pol.load_named(fx.perturb_weights({k: v.float().numpy() for k, v in ref.export_named().items()}, 1, scale=0.25))
    G, C, Bp = 8, 16, 2
    cd = thm._oracle_cfg_dict(cfg)
    grids = [(1, 16, 16), (1, 16, 12)]
    ids, mask = fx.left_pad([fx.synth_prompt(grids[0], 37, cd, 5), fx.synth_prompt(grids[1], 21, cd, 6)], cfg.pad_token_id)
    batch = {"input_ids": ids, "attention_mask": mask, "pixel_values": fx.synth_pixel_values(grids, cd, seed=5), "image_grid_thw": grids}
    eng = SCGRPOEngine(cfg, pol, ref, GRPOArgs(num_generations=G, max_prompt_length=4096, max_completion_length=C, micro_batch_seqs=Bp * G, seed=11, rollout_logps=True))
    try:
        out = _step(eng, batch)
    except RuntimeError as exc:
        if overlap_cus != "0" and "no stream pair" in str(exc):
            pytest.skip(f"co-scheduled case NOT RUN on this box: {exc}")
        raise
    assert eng.last_step_traced and eng.last_step_shadowed == (overlap_cus != "0")
    S, N = ids.shape[1], Bp * G
    hf = eng.pol._ws["carry"]["hf"]
    rows = np.empty((N, C), dtype=np.int64)
    for s in range(N):
        rows[s, 0] = (s // G) * S + S - 1
        rows[s, 1:] = Bp * S + s * C + np.arange(C - 1)
    h = hf[torch.from_numpy(rows.reshape(-1)).to(DEV)].double().cpu()
    W = pol.w(pol.lm_head_name()).double().cpu()
    logits = h @ W.t()
    tok = torch.from_numpy(np.asarray(out["completion_ids"]).reshape(-1, 1))
    want = (logits.gather(1, tok).squeeze(1) - torch.logsumexp(logits, -1)).view(N, C)
    got = out["rollout_logps"].double().cpu()
    keep = torch.from_numpy(np.asarray(out["completion_mask"]).astype(bool))
    K = cfg.hidden_size
    bound = 2 * (1e-4 * logits.abs().max(-1).values.view(N, C) + 1e-3 * math.sqrt(K) * 0.1)
    err = (got - want).abs()
    print(f"[rollout logps] 3B widths, IADR1_OVERLAP_CUS={overlap_cus}: max |sampled - float64| {err[keep].max().item():.3e} (bound >= {bound.min().item():.3e}); metrics "
          f"{ {k: v for k, v in out['metrics'].items() if k.startswith('rollout/')} }")
    assert bool((err[keep] <= bound[keep]).all()), (err[keep].max().item(), bound.min().item())
    assert out["metrics"]["rollout/logp_abs_diff_max"] <= 2 * bound.max().item()
    _SEQUENTIAL[overlap_cus] = got.numpy()
    if overlap_cus != "0" and "0" in _SEQUENTIAL:
        assert np.array_equal(_SEQUENTIAL["0"], got.numpy()), "sequential and co-scheduled steps returned different rollout log-probs"


def test_sampling_generator_and_llava_script_with_temperature(tmp_path, monkeypatch):
    """(10) GreedyGenerator(..., temperature=0.8, seed=6666) on the TINY checkpoint: reproducible, ids in vocabulary, different from the greedy ids somewhere.  The
    LLaVA-OneVision case of test_llava_evaluation_scripts_end_to_end with `--temperature 0.8`: writes its answers file and accuracy csv instead of exiting, and a
    second run from scratch (--reproduce) writes the same answers."""
    import transformers
    import test_entry_e2e as e2e
    from iadr1_amd.evaluate import GreedyGenerator
    from iadr1_amd.trainer import save_checkpoint
    frozen = ParamStore(CFG, DEV, trainable=False, with_decode_pack=True)
    frozen.load_named(fx.make_weights(fx.TINY, 0))
    b = tiny_batch()
    greedy = GreedyGenerator(CFG, frozen, max_new_tokens=12).generate(b)
    s1 = GreedyGenerator(CFG, frozen, max_new_tokens=12, temperature=0.8, seed=6666).generate(b)
    s2 = GreedyGenerator(CFG, frozen, max_new_tokens=12, temperature=0.8, seed=6666).generate(b)
    assert np.array_equal(s1, s2) and s1.min() >= 0 and s1.max() < fx.TINY["text"]["vocab_size"] and not np.array_equal(s1, greedy)
    proc = fx.local_llava_ov_processor()
    tok = proc.tokenizer
    d = dict(fx.TINY_OV, image_token_id=tok.convert_tokens_to_ids("<image>"), eos_token_id=tok.eos_token_id, pad_token_id=tok.pad_token_id)
    t, v = d["text"], d["vision"]
    hfc = {"model_type": "llava_onevision", "architectures": ["LlavaOnevisionForConditionalGeneration"], "image_token_index": d["image_token_id"],
           "image_grid_pinpoints": [list(p) for p in d["image_grid_pinpoints"]], "vision_aspect_ratio": "anyres_max_9", "vision_feature_layer": -1,
           "vision_feature_select_strategy": "full", "tie_word_embeddings": False,
           "text_config": {"model_type": "qwen2", "vocab_size": t["vocab_size"], "hidden_size": t["hidden_size"], "intermediate_size": t["intermediate_size"],
                           "num_hidden_layers": t["num_hidden_layers"], "num_attention_heads": t["num_attention_heads"], "num_key_value_heads": t["num_key_value_heads"],
                           "rms_norm_eps": t["rms_norm_eps"], "rope_theta": t["rope_theta"], "eos_token_id": d["eos_token_id"], "pad_token_id": d["pad_token_id"]},
           "vision_config": {"model_type": "siglip_vision_model", "num_hidden_layers": v["depth"], "hidden_size": v["hidden_size"], "intermediate_size": v["intermediate_size"],
                             "num_attention_heads": v["num_heads"], "num_channels": v["in_channels"], "patch_size": v["patch_size"], "image_size": v["image_size"], "layer_norm_eps": 1e-6}}
    name = "llava-onevision-tiny-si"
    proc.save_pretrained = lambda *a, **k: None
    monkeypatch.setattr(transformers.AutoProcessor, "from_pretrained", classmethod(lambda cls, *a, **k: proc))
    src = str(tmp_path / name)
    s0 = ParamStore(VLMConfig.from_dict(d), DEV, trainable=False)
    s0.load_named(fx.make_weights_ov(d, 0))
    save_checkpoint(s0, src, hfc)
    data = tmp_path / "Industrial_test"
    (data / "MVTec" / "bottle").mkdir(parents=True)
    fx.synth_pil_image(100, 80, 5).save(str(data / "MVTec" / "bottle" / "template.png"))
    chat = {}
    for i in range(3):
        rel = f"MVTec/bottle/{'good' if i == 0 else 'broken'}_{i}.png"
        im = fx.synth_pil_image(100 + 20 * i, 80, 90 + i)
        (im.convert("L") if i == 1 else im).save(str(data / rel))
        chat[rel] = {"conversation": [{"Question": "Is there any defect in the object?", "Answer": "B" if i == 0 else "A", "Options": {"A": "Yes.", "B": "No."}, "type": "Anomaly Detection"}],
                     "similar_templates": ["MVTec/bottle/template.png"], "random_templates": ["MVTec/bottle/template.png"]}
    qfile = tmp_path / "test_data_format.json"
    qfile.write_text(json.dumps(chat))
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr("iadr1_amd.evaluate.GreedyGenerator.__init__", e2e._short_generator_init(), raising=True)
    seen = []
    from iadr1_amd import evaluate
    orig_gen = evaluate.GreedyGenerator.generate
    monkeypatch.setattr(evaluate.GreedyGenerator, "generate", lambda self, batch: (seen.append((self.temperature, self.seed)), orig_gen(self, batch))[1])
    m = e2e._load("scripts/Inference/IAD-R1-Inference/hip_llava_detect_format.py")
    argv = ["x", "--model-path", src, "--test_dataset", "test_data", "--json_path", str(qfile), "--data_path", str(data), "--batch_size", "2", "--temperature", "0.8"]
    monkeypatch.setattr(sys, "argv", argv)
    m.main()
    ans_path = tmp_path / "result" / "LlaVA" / "test_data" / f"answers_1_shot_{name}_vllm.json"
    answers = json.load(open(ans_path))
    assert [a["image"] for a in answers] == list(chat) and all(a["gpt_answer"] for a in answers)
    assert os.path.exists(str(ans_path).replace(".json", "_accuracy.csv")) and seen == [(0.8, 6666), (0.8, 6666)]
    monkeypatch.setattr(sys, "argv", argv + ["--reproduce"])
    m.main()
    assert json.load(open(ans_path)) == answers and len(seen) == 4


@pytest.mark.parametrize("batched", [True, False])
def test_trainer_logs_the_metrics_also_with_batched_rollouts(tmp_path, batched):
    """GRPOConfig.rollout_logps through SCGRPOTrainer.training_step, three micro-batches: with one rollout for all of them (batch_rollouts: the log-probs are handed
    to each micro-batch's step with its completions) and with one rollout per micro-batch, every micro-batch logs the three metrics, finite; the flag off logs none."""
    from iadr1_amd import rewards, rollout as ro
    from iadr1_amd.trainer import GRPOConfig, SCGRPOTrainer
    w = fx.make_weights(fx.TINY, 0)
    grids = [(1, 16, 12), (1, 8, 8), (1, 12, 12)]
    parts = []
    for i, (gr, n) in enumerate(zip(grids, [5, 17, 9])):
        ids, mask = fx.left_pad([fx.synth_prompt(gr, n, fx.TINY, 177 + i)], fx.TINY["pad_token_id"])
        parts.append({"input_ids": ids, "attention_mask": mask, "pixel_values": torch.from_numpy(fx.synth_pixel_values([gr], fx.TINY, seed=177 + i)), "image_grid_thw": [gr]})

    class Proc:
        def apply_chat_template(self, conv, add_generation_prompt=True, tokenize=False):
            return "P"

        def __call__(self, text=None, images=None, **kw):
            return parts[images[0][1]]

        def batch_decode(self, ids, skip_special_tokens=True):
            return ["<think>a</think><location>top left</location><type>scratch</type><answer>yes</answer>"] * len(ids)
    chat = [{"role": "user", "content": [{"type": "image"}, {"type": "text", "text": "?"}]}]
    rows = lambda k: [{"prompt": chat, "image": [("synthetic", k)], "solution": "<think>gt</think><location>top left</location><type>scratch</type><answer>yes</answer>"}]
    keys = ("rollout/logp_abs_diff_mean", "rollout/logp_abs_diff_max", "rollout/kl")
    for flag in (True, False):
        tr = SCGRPOTrainer((CFG, w), [rewards.accuracy_reward, rewards.consistency_reward], processing_class=Proc(), train_dataset=None,
                           args=GRPOConfig(output_dir=str(tmp_path / "out"), num_generations=4, max_completion_length=12, max_prompt_length=4096,
                                           per_device_train_batch_size=1, gradient_accumulation_steps=3, save_steps=0, batch_rollouts=batched, rollout_logps=flag))
        n0 = ro.STATS["rollouts"]
        losses = tr.training_step([rows(0), rows(1), rows(2)])
        assert ro.STATS["rollouts"] - n0 == (1 if batched else 3) and len(losses) == 3 and all(np.isfinite(l) for l in losses)
        if flag:
            assert all(len(tr._metrics[k]) == 3 and all(np.isfinite(v) and v >= 0 for v in tr._metrics[k]) for k in keys), dict(tr._metrics)
            tr.log({"loss": float(np.mean(losses))})
            assert all(k in tr.log_history[-1] for k in keys)
        else:
            assert not any(k in tr._metrics for k in keys)
