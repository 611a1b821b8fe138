"""The rollout returns the entropy of the distribution every token was sampled from (Rollout.generate(return_entropy=True), GRPOArgs.rollout_entropy), the engine
logs its mean as `entropy`, and the trainer carries it -- and the top_entropy_quantile mask drawn from it -- through batched rollouts and reuse steps.  GPU only.
Fixture and helpers are those of tests/test_rollout_logps.py."""
import dataclasses
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
import test_rollout_logps as trl_  # noqa: E402  (stores, tiny_batch, reward_fn, _step)
from iadr1_amd.params import ParamStore, VLMConfig  # noqa: E402
from iadr1_amd.sc_grpo import GRPOArgs, SCGRPOEngine  # noqa: E402

DEV = "cuda"
CFG = trl_.CFG
LN_V = math.log(fx.TINY["text"]["vocab_size"])


def roll(cfg=CFG, **kw):
    pol, ref = trl_.stores(cfg)
    eng = SCGRPOEngine(cfg, pol, ref, GRPOArgs(num_generations=4, max_prompt_length=4096, max_completion_length=16, seed=5, **kw))
    toks = eng.rollout(trl_.tiny_batch())
    host = lambda t: None if t is None else t.cpu().numpy()
    return toks, host(eng.last_rollout_logps), host(eng.last_rollout_entropy)


def live_positions(toks, eos):
    live = np.ones_like(toks, dtype=bool)
    for r in range(toks.shape[0]):
        e = np.flatnonzero(toks[r] == eos)
        if e.size:
            live[r, e[0] + 1:] = False
    return live


def test_rollout_returns_entropies_without_changing_tokens_or_logps():
    """Tokens and log-probs bit-equal with the flag on and off; entropies bit-equal between graph and eager and between two runs; 0 <= H <= ln V + 1e-4 at every live
    position; zeros after a sequence's first EOS; the same with the whole-vocabulary draw and with the penalty / min_p sampler."""
    t0, lp0, none = roll(rollout_logps=True)
    assert none is None
    t1, lp1, h1 = roll(rollout_logps=True, rollout_entropy=True)
    t2, lp2, h2 = roll(rollout_logps=True, rollout_entropy=True)
    t3, lp3, h3 = roll(rollout_logps=True, rollout_entropy=True, use_hip_graph=False)
    t4, none4, h4 = roll(rollout_entropy=True)
    t5, _, none5 = roll()
    assert none4 is None and none5 is None
    for t in (t1, t2, t3, t4, t5):
        assert np.array_equal(t0, t)
    assert np.array_equal(lp0, lp1) and np.array_equal(lp0, lp2) and np.array_equal(lp0, lp3)
    assert h1.shape == t1.shape and h1.dtype == np.float32 and np.array_equal(h1, h2) and np.array_equal(h1, h3) and np.array_equal(h1, h4)
    live = live_positions(t1, CFG.eos_token_id)
    print(f"[rollout entropy] TINY: H in [{h1[live].min():.4f}, {h1[live].max():.4f}], mean {h1[live].mean():.4f}, ln V = {LN_V:.4f}")
    assert np.isfinite(h1).all() and (h1[live] >= 0).all() and (h1[live] <= LN_V + 1e-4).all() and (h1[live] > 0).any() and (h1[~live] == 0).all()
    # EOS: declare a token the sampler draws in the middle of some rows to be EOS; sampling is a pure function of (seed, step, row, logits)
    best = max(np.unique(t1[:, 2:12]), key=lambda tok: sum(tok in t1[r, 2:12] and tok not in t1[r, :2] for r in range(t1.shape[0])))
    cfg2 = dataclasses.replace(CFG, eos_token_id=int(best))
    te, lpe, he = roll(cfg2, rollout_logps=True, rollout_entropy=True)
    ended = 0
    for r in range(te.shape[0]):
        e = np.flatnonzero(te[r] == best)
        n = e[0] + 1 if e.size else te.shape[1]
        ended += bool(e.size) and n < te.shape[1]
        assert np.array_equal(te[r, :n], t1[r, :n]) and np.array_equal(he[r, :n], h1[r, :n]) and (he[r, n:] == 0).all() and (lpe[r, n:] == 0).all(), r
    assert ended > 0
    # the other sampler paths: the entropy is the raw row's whatever the filter does, the tokens are those of the rollout without the flag
    for kw in (dict(top_k=0, top_p=1.0), dict(min_p=0.05, repetition_penalty=1.3)):
        a, la, ha = roll(rollout_logps=True, rollout_entropy=True, **kw)
        b, lb, _ = roll(rollout_logps=True, **kw)
        assert np.array_equal(a, b) and np.array_equal(la, lb), kw
        lv = live_positions(a, CFG.eos_token_id)
        assert (ha[lv] >= 0).all() and (ha[lv] <= LN_V + 1e-4).all() and (ha[~lv] == 0).all()
        assert np.array_equal(ha[:, 0], h1[:, 0]), "token 0 is sampled from the same prefill logits under every filter"


def test_toggling_the_flag_recaptures_and_the_default_launches_stay():
    """One engine, flag off -> on -> off by hand on its Rollout: the `entropy` key of the sampling dict invalidates the captured graph both ways, the tokens stay, and
    with the flag off the sampler branch taken is the one taken before (no entropy buffer is touched)."""
    from iadr1_amd import rollout as ro
    pol, ref = trl_.stores()
    eng = SCGRPOEngine(CFG, pol, ref, GRPOArgs(num_generations=4, max_prompt_length=4096, max_completion_length=16, seed=5))
    t0 = eng.rollout(trl_.tiny_batch()).copy()
    r = eng._rollout
    assert r.entropy is None and r.sampling["entropy"] is False
    n0 = ro.STATS["graph_captures"]
    eng.args.rollout_entropy = True
    t1 = eng.rollout(trl_.tiny_batch()).copy()
    assert ro.STATS["graph_captures"] == n0 + 1 and r.sampling["entropy"] is True and np.array_equal(t0, t1)
    h = eng.last_rollout_entropy.clone()
    eng.args.rollout_entropy = False
    r.entropy.fill_(-3.0)
    t2 = eng.rollout(trl_.tiny_batch()).copy()
    assert ro.STATS["graph_captures"] == n0 + 2 and eng.last_rollout_entropy is None and np.array_equal(t0, t2) and bool((r.entropy == -3.0).all())
    eng.args.rollout_entropy = True
    eng.rollout(trl_.tiny_batch())
    assert torch.equal(eng.last_rollout_entropy, h)


def test_engine_step_metric_leaves_the_step_unchanged():
    """SCGRPOEngine.step with rollout_entropy=True: loss, completion ids, logps, kl and the gradients bit-equal to the step with the flag off; the metric key set gains
    exactly `entropy`, the result exactly "rollout_entropy"; the metric is the float64 mean over the EOS mask."""
    batch = trl_.tiny_batch()
    res = {}
    for flag in (False, True):
        pol, ref = trl_.stores()
        eng = SCGRPOEngine(CFG, pol, ref, GRPOArgs(num_generations=4, max_prompt_length=4096, max_completion_length=16, seed=5, rollout_entropy=flag))
        out = trl_._step(eng, batch)
        res[flag] = (out, pol.grad.clone())
    (o0, g0), (o1, g1) = res[False], res[True]
    assert o0["metrics"]["loss"] == o1["metrics"]["loss"] and o0["metrics"]["kl"] == o1["metrics"]["kl"]
    assert np.array_equal(o0["completion_ids"], o1["completion_ids"]) and torch.equal(o0["logps"], o1["logps"]) and torch.equal(o0["kl"], o1["kl"]) and torch.equal(g0, g1)
    assert set(o1["metrics"]) == set(o0["metrics"]) | {"entropy"} and "entropy" not in o0["metrics"]
    assert set(o1) == set(o0) | {"rollout_entropy"} and "rollout_entropy" not in o0 and "entropy_mask" not in o1
    h = o1["rollout_entropy"].double().cpu().numpy()
    live = live_positions(np.asarray(o1["completion_ids"]), CFG.eos_token_id)
    print(f"[rollout entropy] TINY step: entropy {o1['metrics']['entropy']:.6f}")
    assert tuple(h.shape) == tuple(o1["logps"].shape) and abs(o1["metrics"]["entropy"] - h[live].mean()) <= 1e-5 * h[live].mean()


def test_rollout_entropy_against_float64_from_the_stored_final_norm_rows(monkeypatch):
    """The 2-layer model at 3B widths of test_rollout_logps_against_float64_from_the_stored_final_norm_rows, sequential case: H64 from `hf @ W.T` in float64 over the
    final-norm rows the decode steps stored.  Bound per token: 2 * delta * sum_v p_v |ln p_v + H| -- delta is that test's bound on a decode logit (rtol 1e-4 of
    max |logit| + 1e-3 * sqrt(K) * 0.1), the sum is the float64 first-order sensitivity of H to a sup-norm logit error (dH/dx_v = -p_v (ln p_v + H)), the factor 2
    covers the second order."""
    import test_hip_model as thm
    monkeypatch.setenv("IADR1_OVERLAP_CUS", "0")
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
    eng = SCGRPOEngine(cfg, pol, ref, GRPOArgs(num_generations=G, max_prompt_length=4096, max_completion_length=C, micro_batch_seqs=Bp * G, seed=11, rollout_logps=True,
                                               rollout_entropy=True))
    out = trl_._step(eng, batch)
    assert eng.last_step_traced and not eng.last_step_shadowed
    S, N = ids.shape[1], Bp * G
    hf = eng.pol._ws["carry"]["hf"]
    rows = np.empty((N, C), dtype=np.int64)
    for s in range(N):
        rows[s, 0] = (s // G) * S + S - 1
        rows[s, 1:] = Bp * S + s * C + np.arange(C - 1)
    h = hf[torch.from_numpy(rows.reshape(-1)).to(DEV)].double().cpu()
    W = pol.w(pol.lm_head_name()).double().cpu()
    logits = h @ W.t()
    lnp = torch.log_softmax(logits, -1)
    p = lnp.exp()
    H64 = -(p * lnp).sum(-1)
    sens = (p * (lnp + H64[:, None]).abs()).sum(-1).view(N, C)
    H64 = H64.view(N, C)
    got = out["rollout_entropy"].double().cpu()
    keep = torch.from_numpy(np.asarray(out["completion_mask"]).astype(bool))
    K = cfg.hidden_size
    delta = 1e-4 * logits.abs().max(-1).values.view(N, C) + 1e-3 * math.sqrt(K) * 0.1
    bound = 2 * delta * sens
    err = (got - H64).abs()
    print(f"[rollout entropy] 3B widths: max |H - H64| {err[keep].max().item():.3e}, max err / bound {(err[keep] / bound[keep]).max().item():.3f} (bound in "
          f"[{bound[keep].min().item():.3e}, {bound[keep].max().item():.3e}]); H64 in [{H64[keep].min().item():.3f}, {H64[keep].max().item():.3f}]; entropy metric "
          f"{out['metrics']['entropy']:.5f}")
    assert bool((err[keep] <= bound[keep]).all()), (err[keep].max().item(), bound[keep].min().item())
    assert abs(out["metrics"]["entropy"] - H64[keep].mean().item()) <= bound[keep].max().item()


class _Proc:
    def __init__(self, parts):
        self.parts = parts

    def apply_chat_template(self, conv, add_generation_prompt=True, tokenize=False):
        return "P"

    def __call__(self, text=None, images=None, **kw):
        return self.parts[images[0][1]]

    def batch_decode(self, ids, skip_special_tokens=True):
        return ["<think>a</think><location>top left</location><type>scratch</type><answer>yes</answer>"] * len(ids)


def _trainer(tmp_path, **kw):
    from iadr1_amd import rewards
    from iadr1_amd.trainer import GRPOConfig, SCGRPOTrainer
    w = fx.make_weights(fx.TINY, 0)
    grids = [(1, 16, 12), (1, 8, 8), (1, 12, 12)]
    parts = []
    for i, (gr, n) in enumerate(zip(grids, [5, 17, 9])):
        ids, mask = fx.left_pad([fx.synth_prompt(gr, n, fx.TINY, 177 + i)], fx.TINY["pad_token_id"])
        parts.append({"input_ids": ids, "attention_mask": mask, "pixel_values": torch.from_numpy(fx.synth_pixel_values([gr], fx.TINY, seed=177 + i)), "image_grid_thw": [gr]})
    chat = [{"role": "user", "content": [{"type": "image"}, {"type": "text", "text": "?"}]}]
    rows = lambda k: [{"prompt": chat, "image": [("synthetic", k)], "solution": "<think>gt</think><location>top left</location><type>scratch</type><answer>yes</answer>"}]
    tr = SCGRPOTrainer((CFG, w), [rewards.accuracy_reward, rewards.consistency_reward], processing_class=_Proc(parts), train_dataset=None,
                       args=GRPOConfig(output_dir=str(tmp_path / "out"), num_generations=4, max_completion_length=12, max_prompt_length=4096,
                                       per_device_train_batch_size=1, gradient_accumulation_steps=3, save_steps=0, **kw))
    return tr, [rows(0), rows(1), rows(2)]


@pytest.mark.parametrize("batched", [True, False])
def test_trainer_logs_the_entropy_also_with_batched_rollouts(tmp_path, batched):
    """GRPOConfig.rollout_entropy through SCGRPOTrainer.training_step, three micro-batches, one rollout for all of them or one each: every micro-batch logs `entropy`,
    in (0, ln V]; the flag off logs none."""
    from iadr1_amd import rollout as ro
    for flag in (True, False):
        tr, mbs = _trainer(tmp_path, batch_rollouts=batched, rollout_entropy=flag)
        n0 = ro.STATS["rollouts"]
        losses = tr.training_step(mbs)
        assert ro.STATS["rollouts"] - n0 == (1 if batched else 3) and len(losses) == 3 and all(np.isfinite(l) for l in losses)
        if flag:
            assert len(tr._metrics["entropy"]) == 3 and all(0 < v <= LN_V + 1e-4 for v in tr._metrics["entropy"]), dict(tr._metrics)
            tr.log({"loss": float(np.mean(losses))})
            assert "entropy" in tr.log_history[-1] and not any(k.startswith("entropy/") for k in tr.log_history[-1])
        else:
            assert not any(k.startswith("entropy") for k in tr._metrics)


@pytest.mark.parametrize("batched", [True, False])
def test_reuse_step_logs_no_entropy_and_applies_the_cached_mask(tmp_path, batched, monkeypatch):
    """num_iterations = 2 with top_entropy_quantile = 0.5: step 0 logs entropy, entropy/threshold and entropy/kept_frac once per micro-batch and caches entropies and
    mask; the reuse step logs none of them and hands every micro-batch's cached mask to the loss (the selector the kernel gets is that mask, bit for bit)."""
    from iadr1_amd import ops
    tr, mbs = _trainer(tmp_path, batch_rollouts=batched, top_entropy_quantile=0.5, num_iterations=2, learning_rate=1e-3)
    keys = ("entropy", "entropy/threshold", "entropy/kept_frac")
    tr.training_step(mbs)
    assert all(len(tr._metrics[k]) == 3 for k in keys), dict(tr._metrics)
    assert len(tr._generation) == 3
    for g in tr._generation:
        c = g["completions"].shape[1]
        assert g["entropy_mask"].dtype == torch.bool and tuple(g["entropy_mask"].shape) == (4, c) == tuple(g["rollout_entropy"].shape) and bool(g["entropy_mask"].any())
    tr._metrics.clear()
    seen = []
    orig = ops.grpo_loss_ex
    monkeypatch.setattr(ops, "grpo_loss_ex", lambda *a, **k: (seen.append((k.get("sel"), k.get("old_logp"))), orig(*a, **k))[1])
    losses = tr.training_step(None)
    assert len(losses) == 3 and all(np.isfinite(l) for l in losses) and not any(k in tr._metrics for k in keys) and "clip_ratio/region_mean" in tr._metrics
    assert len(seen) == 3
    for (sel, old), g in zip(seen, tr._generation):
        assert old is not None and sel is not None and torch.equal(sel.bool(), g["entropy_mask"])
    # a reuse step whose cache lost its mask is refused by name
    tr.state.global_step = 1
    tr._generation[0]["entropy_mask"] = None
    with pytest.raises(ValueError, match="top_entropy_quantile < 1: a reuse iteration .* needs the entropy_mask"):
        tr.training_step(None)
