"""GRPOArgs.logps_at_temperature through SCGRPOEngine: the policy's and the reference's log-probs, the cached old_logps, the rollout's log-probs and entropies all
under softmax(x / temperature); the default untouched.  GPU only; the kernel-level checks are test_logp_temperature's.

The exact check: at temperature 0.5 the option is the plain step on a model whose (untied) lm_head is doubled -- y = x / 0.5 = 2 x is what a doubled bf16 weight
contracts to, bit for bit -- so log-probs, loss and kl of the two steps are equal bits, every gradient but the lm_head's as well, and the lm_head's is exactly twice
(dlogits carries the chain rule's 1 / T = 2)."""
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
import test_grpo_objective as tgo  # noqa: E402  (RAGGED, completions, formula)
import test_rollout_is as tri  # noqa: E402  (stores, tiny_batch, reward_fn, close)
from iadr1_amd import ops, sc_grpo  # noqa: E402
from iadr1_amd.params import ParamStore, VLMConfig  # noqa: E402
from iadr1_amd.sc_grpo import GRPOArgs, SCGRPOEngine  # noqa: E402

DEV = "cuda"
F32 = torch.float32
CFG = tri.CFG
CFG7 = VLMConfig.from_dict(fx.TINY7)
G, C = tgo.G, tgo.C_ENG
BETA = tri.BETA
T = 0.9


# ---- exact: temperature 0.5 is a doubled lm_head ---------------------------------------------------------------------------------------------------------------

def stores7(double_head):
    """Policy (perturbed) and frozen reference of the untied fixture; double_head: both lm_heads times 2 (exact in bf16)."""
    w = fx.make_weights(fx.TINY7, 0)
    wp = fx.perturb_weights(w, 1, scale=0.25)
    if double_head:
        w, wp = dict(w), dict(wp)
        w["lm_head.weight"], wp["lm_head.weight"] = w["lm_head.weight"] * 2, wp["lm_head.weight"] * 2
    pol, ref = ParamStore(CFG7, DEV, trainable=True), ParamStore(CFG7, DEV, trainable=False)
    pol.load_named(wp)
    ref.load_named(w)
    return pol, ref


def batch7():
    grids = [(1, 16, 12), (1, 8, 8)]
    rows = [fx.synth_prompt(gr, n, fx.TINY7, 77 + i) for i, (gr, n) in enumerate(zip(grids, [5, 17]))]
    ids, mask = fx.left_pad(rows, fx.TINY7["pad_token_id"])
    return {"input_ids": ids, "attention_mask": mask, "pixel_values": fx.synth_pixel_values(grids, fx.TINY7, seed=77), "image_grid_thw": grids}


def scored7(comp, double_head, **kw):
    pol, ref = stores7(double_head)
    eng = SCGRPOEngine(CFG7, pol, ref, GRPOArgs(num_generations=G, max_prompt_length=4096, max_completion_length=C, seed=5, **kw))
    out = eng.loss_and_grads(batch7(), comp, tri.reward_fn(comp))
    torch.cuda.synchronize()
    return out, pol


@pytest.mark.parametrize("mbs", [16, G])
def test_half_temperature_is_the_plain_step_on_a_doubled_lm_head(mbs):
    comp = sc_grpo.right_pad(fx.synth_completions(2 * G, C, fx.TINY7, 321, tgo.RAGGED), CFG7.pad_token_id)
    A, pa = scored7(comp, False, logps_at_temperature=True, temperature=0.5, micro_batch_seqs=mbs)
    B, pb = scored7(comp, True, temperature=0.5, micro_batch_seqs=mbs)
    assert pa.lm_head_name() == "lm_head" and np.array_equal(A["completion_mask"], B["completion_mask"])
    for k in ("logps", "ref_logps"):
        assert torch.equal(A[k], B[k]), k
    assert A["metrics"]["loss"] == B["metrics"]["loss"] and A["metrics"]["kl"] == B["metrics"]["kl"] and A["metrics"]["kl"] > 0
    head = pa.g("lm_head")
    assert float(head.abs().max()) > 0 and torch.equal(head, 2 * pb.g("lm_head")), "the lm_head gradient is exactly twice the doubled run's"
    s = pa.slots["lm_head"]
    n = int(np.prod(s.shape))
    rest = torch.ones(pa.grad.numel(), dtype=torch.bool, device=DEV)
    rest[s.offset: s.offset + n] = False
    assert torch.equal(pa.grad[rest], pb.grad[rest]) and float(pa.grad[rest].abs().max()) > 0, "every other gradient is bit-equal"
    # the option did something: the plain step on the same weights scores other numbers
    P, _ = scored7(comp, False, temperature=0.5, micro_batch_seqs=mbs)
    live = torch.from_numpy(np.asarray(A["completion_mask"]).astype(bool)).to(DEV)
    assert float((A["logps"] - P["logps"])[live].abs().max()) > 1e-3


# ---- the tied fixture at temperature 0.9 ---------------------------------------------------------------------------------------------------------------------------

def scored(comp, **kw):
    call = {k: kw.pop(k) for k in ("ref_logps", "old_logps") if k in kw}
    pol, ref = tri.stores()
    eng = SCGRPOEngine(CFG, pol, ref, GRPOArgs(num_generations=G, max_prompt_length=4096, max_completion_length=C, seed=5, **kw))
    out = eng.loss_and_grads(tri.tiny_batch(), comp, tri.reward_fn(comp), **call)
    torch.cuda.synchronize()
    return out, pol.grad.clone(), eng


@pytest.fixture(scope="module")
def tied():
    """(completions, the step with the option on at T = 0.9, the step with it off)"""
    comp = tgo.completions(tgo.RAGGED)
    return comp, scored(comp, logps_at_temperature=True, temperature=T), scored(comp, temperature=T)


@pytest.mark.parametrize("loss_type", tgo.LOSS_TYPES)
def test_loss_is_the_trl_formula_on_the_scaled_logps(tied, loss_type):
    comp, (on, _, _), (off, _, _) = tied
    if loss_type != "grpo":
        on, _, _ = scored(comp, logps_at_temperature=True, temperature=T, loss_type=loss_type)
    want = tgo.formula(on, loss_type, BETA)
    print(f"[logp_temperature engine] {loss_type}: loss {on['metrics']['loss']:.9e} float64 {want:.9e}")
    tri.close(torch.tensor(on["metrics"]["loss"]), torch.tensor(want), 1e-5, 1e-7, f"{loss_type}: loss")
    live = torch.from_numpy(np.asarray(on["completion_mask"]).astype(bool)).to(DEV)
    for k in ("logps", "ref_logps"):
        assert float((on[k] - off[k])[live].abs().max()) > 1e-3, f"{k}: the switch reaches the kernel"


def test_the_scaled_logps_are_the_fused_lm_head_at_that_temperature_and_the_default_is_the_old_entry_point(tied):
    """The step's log-probs against ops.linear_logprob on the rows the step scored: with the option on at `temperature`, with it off at temperature=1.0 -- the old
    entry point, the launch of an engine built before the attribute existed."""
    comp, (on, _, eng_on), (off, g_off, eng_off) = tied
    assert eng_on.pol.logp_temperature == T and eng_on.ref.logp_temperature == T and eng_off.pol.logp_temperature == 1.0 and eng_off.ref.logp_temperature == 1.0
    for out, eng, temp in ((on, eng_on, T), (off, eng_off, 1.0)):
        seen = []
        real = ops.linear_logprob

        def spy(h, w, targets, logp=None, lse=None, ws=None, temperature=1.0):
            res = real(h, w, targets, logp=logp, lse=lse, ws=ws, temperature=temperature)
            again = real(h, w, targets, temperature=temp)          # 1.0: iadr1_linear_logprob_fwd itself
            seen.append((temperature, torch.equal(res[0], again[0]) and torch.equal(res[1], again[1])))
            return res
        ops.linear_logprob = spy
        try:
            out2 = eng.loss_and_grads(tri.tiny_batch(), comp, tri.reward_fn(comp))
            torch.cuda.synchronize()
        finally:
            ops.linear_logprob = real
        assert len(seen) >= 2 and all(t == temp and same for t, same in seen), seen          # the policy's pass and the reference's
        assert torch.equal(out2["logps"], out["logps"]) and torch.equal(out2["ref_logps"], out["ref_logps"])
    assert float(g_off.abs().max()) > 0


def test_reuse_step_reads_the_scaled_old_logps(tied):
    """num_iterations 2 at unchanged weights: old_logps are step 0's returned (T-scaled) log-probs, every ratio is exactly 1 and nothing is clipped."""
    comp, (o0, g0, _), (off, _, _) = tied
    o1, g1, _ = scored(comp, logps_at_temperature=True, temperature=T, num_iterations=2, old_logps=o0["logps"], ref_logps=o0["ref_logps"])
    m = o1["metrics"]
    assert torch.equal(o1["old_logps"], o0["logps"]) and torch.equal(o1["logps"], o0["logps"]) and not torch.equal(o0["logps"], off["logps"])
    # (every ratio is exactly 1: logp_abs_diff_max is 0; their mean goes through 1 / count per ragged row, held to test_grpo_clip's 1e-5)
    assert abs(m["policy/ratio_mean"] - 1.0) <= 1e-5 and m["policy/logp_abs_diff_max"] == 0.0 and m["clip_ratio/region_mean"] == 0.0
    assert m["loss"] == o0["metrics"]["loss"] and m["kl"] == o0["metrics"]["kl"] and torch.equal(g0, g1)
    # against old log-probs at temperature 1 the same weights would show a ratio: that is the mismatch the option removes
    o2, _, _ = scored(comp, logps_at_temperature=True, temperature=T, num_iterations=2, old_logps=off["logps"], ref_logps=o0["ref_logps"])
    assert o2["metrics"]["policy/logp_abs_diff_max"] > 1e-3


# ---- the rollout ---------------------------------------------------------------------------------------------------------------------------------------------------

def roll(**kw):
    pol, ref = tri.stores()
    eng = SCGRPOEngine(CFG, pol, ref, GRPOArgs(num_generations=4, max_prompt_length=4096, max_completion_length=16, seed=5, temperature=T, **kw))
    toks = eng.rollout(tri.tiny_batch())
    torch.cuda.synchronize()
    lp, en = eng.last_rollout_logps, eng.last_rollout_entropy
    return toks, None if lp is None else lp.cpu().numpy(), None if en is None else en.cpu().numpy(), eng


def test_rollout_tokens_do_not_change_and_graph_equals_eager():
    t0, lp0, en0, _ = roll(rollout_logps=True, rollout_entropy=True)
    t1, lp1, en1, e1 = roll(rollout_logps=True, rollout_entropy=True, logps_at_temperature=True)
    t2, lp2, en2, _ = roll(rollout_logps=True, rollout_entropy=True, logps_at_temperature=True, use_hip_graph=False)
    t3, lp3, _, _ = roll(rollout_logps=True, logps_at_temperature=True)          # log-probs alone: the same launch without the entropy output
    t4, none, _, e4 = roll(logps_at_temperature=True)                            # neither: the argument changes nothing and the plain sampler runs
    assert np.array_equal(t0, t1) and np.array_equal(t1, t2) and np.array_equal(t1, t3) and np.array_equal(t1, t4) and none is None
    assert np.array_equal(lp1, lp2) and np.array_equal(en1, en2) and np.array_equal(lp1, lp3)
    assert e1._rollout.sampling["logp_temperature"] == T and e4._rollout.sampling["logp_temperature"] == 1.0 and not e4._rollout.sampling["entropy"]
    live = np.ones_like(t1, dtype=bool)
    for r in range(t1.shape[0]):
        e = np.flatnonzero(t1[r] == CFG.eos_token_id)
        if e.size:
            live[r, e[0] + 1:] = False
    assert (lp1[live] < 0).all() and (lp1[~live] == 0).all() and (en1[live] > 0).all() and (en1[~live] == 0).all()
    assert np.abs(lp1 - lp0)[live].max() > 1e-3 and np.abs(en1 - en0)[live].max() > 1e-3


WIDE_ENV = ("IADR1_OVERLAP_CUS", "IADR1_DECODE_KS")


def wide_step(overlap_cus, **kw):
    """tri._wide_step (the 2-layer model at Qwen2.5-VL-3B widths whose decode steps fill the training arena) with other GRPOArgs."""
    import test_hip_model as thm
    os.environ["IADR1_OVERLAP_CUS"] = overlap_cus
    os.environ["IADR1_DECODE_KS"] = "1,8"          # the same split of the o projection's K whatever the CU count (test_rollout_logps)
    cfg = dataclasses.replace(VLMConfig.qwen25vl_3b(), num_hidden_layers=2, v_depth=2, v_fullatt=(1,))
    ref = ParamStore(cfg, DEV, trainable=False)
    ref.init_random(seed=0)
    pol = ParamStore(cfg, DEV, trainable=True)
    pol.load_named(fx.perturb_weights({k: v.float().numpy() for k, v in ref.export_named().items()}, 1, scale=0.25))
    Gw, Cw, Bp = 8, 16, 2
    cd = thm._oracle_cfg_dict(cfg)
    grids = [(1, 16, 16), (1, 16, 12)]
    ids, mask = fx.left_pad([fx.synth_prompt(grids[0], 37, cd, 5), fx.synth_prompt(grids[1], 21, cd, 6)], cfg.pad_token_id)
    batch = {"input_ids": ids, "attention_mask": mask, "pixel_values": fx.synth_pixel_values(grids, cd, seed=5), "image_grid_thw": grids}
    eng = SCGRPOEngine(cfg, pol, ref, GRPOArgs(num_generations=Gw, max_prompt_length=4096, max_completion_length=Cw, micro_batch_seqs=Bp * Gw, seed=11, temperature=T, **kw))
    out = eng.step(batch, tri.reward_fn, do_optimizer_step=False, return_outputs=True)
    torch.cuda.synchronize()
    S, N = ids.shape[1], Bp * Gw
    rows = np.empty((N, Cw), dtype=np.int64)          # the final-norm rows the decode steps stored: column 0 reads the prompt's last row of the prefill
    for s in range(N):
        rows[s, 0] = (s // Gw) * S + S - 1
        rows[s, 1:] = Bp * S + s * Cw + np.arange(Cw - 1)
    return eng, pol, out, torch.from_numpy(rows.reshape(-1)).to(DEV)


@pytest.fixture(scope="module")
def wide():
    """ONE full step at 3B widths with the option, the cap and the entropies on, shared by the two tests below: co-scheduled (IADR1_OVERLAP_CUS forced to 64, as the
    overlap parity tests force it) where the box has a clean stream pair, else sequential.  -> (overlap_cus, engine, policy store, step result, arena rows)"""
    saved = {k: os.environ.get(k) for k in WIDE_ENV}
    try:
        for cus in ("64", "0"):
            try:
                return (cus,) + wide_step(cus, rollout_is_cap=2.0, rollout_entropy=True, logps_at_temperature=True)
            except RuntimeError as exc:
                if cus == "0" or "no stream pair" not in str(exc):
                    raise
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def test_full_step_with_the_cap_compares_two_logps_at_the_same_temperature(wide):
    """rollout_is_cap 2 with the option on: the rollout's log-probs and entropies against float64 from the stored final-norm rows at x / T, inside the bound
    test_rollout_logps derives at temperature 1 times 1 / T (a logit error scales by 1 / T); rollout/logp_abs_diff_max within twice that; the weights and
    rollout/is_weight_mean as test_rollout_is holds them.  The rollout's log-probs at temperature 1 against the same scores would not meet it."""
    cus, eng, pol, out, rows = wide
    assert eng.last_step_traced
    N, Cw = out["completion_ids"].shape
    h = eng.pol._ws["carry"]["hf"][rows].double().cpu()
    logits = h @ pol.w(pol.lm_head_name()).double().cpu().t()
    y = logits / float(np.float32(T))
    tok = torch.from_numpy(np.asarray(out["completion_ids"]).reshape(-1, 1))
    lsm = y - torch.logsumexp(y, -1, keepdim=True)
    want = lsm.gather(1, tok).squeeze(1).view(N, Cw)
    want_h = -(torch.exp(lsm) * lsm).sum(-1).view(N, Cw)
    keep = torch.from_numpy(np.asarray(out["completion_mask"]).astype(bool))
    K = eng.cfg.hidden_size
    bound = 2 * (1e-4 * logits.abs().max(-1).values.view(N, Cw) + 1e-3 * math.sqrt(K) * 0.1) / T
    err = (out["rollout_logps"].double().cpu() - want).abs()
    m = out["metrics"]
    print(f"[logp_temperature engine] 3B widths, IADR1_OVERLAP_CUS={cus}: max |sampled - float64| {err[keep].max().item():.3e} (bound >= {bound.min().item():.3e}); "
          f"{ {k: v for k, v in m.items() if k.startswith('rollout/') or k == 'entropy'} }")
    assert bool((err[keep] <= bound[keep]).all()), (err[keep].max().item(), bound.min().item())
    assert m["rollout/logp_abs_diff_max"] <= 2 * bound.max().item()
    tri._check_weights_against_float64(out, 2.0, "3B widths, logps_at_temperature")
    # the entropies: dH / dy_i = -p_i (ln p_i + H), so |dH| <= (sum p_i |ln p_i| + H) max |dy| = 2 H max |dy| <= 2 ln V max |dy|, and the bound above is 2 max |dy|
    err_h = (out["rollout_entropy"].double().cpu() - want_h).abs()
    assert bool((err_h[keep] <= (bound * math.log(logits.shape[1]))[keep]).all()), err_h[keep].max().item()
    assert abs(m["entropy"] - float(want_h[keep].mean())) <= float(bound.max()) * math.log(logits.shape[1])
    # only the rollout side at temperature 1 (float64, the same rows): its distance to the scores at T is far outside
    lsm1 = logits - torch.logsumexp(logits, -1, keepdim=True)
    mixed = (lsm1.gather(1, tok).squeeze(1).view(N, Cw) - out["logps"].double().cpu()).abs()
    assert float(mixed[keep].max()) > 2 * bound.max().item() + float(err[keep].max())


def test_co_scheduled_policy_head_is_engine_logprobs_bit_for_bit(wide):
    """IADR1_OVERLAP_CUS forced: the side stream's pol_logp (ChunkedRefPass._policy_head) equals Engine.logprobs on the same rows with the option on."""
    cus, eng, pol, out, rows = wide
    if cus == "0":
        pytest.skip("co-scheduled case NOT RUN on this box: no stream pair")
    assert eng.last_step_shadowed and eng.shadow_policy_head is not None and eng.pol.logp_temperature == T
    N, Cw = out["completion_ids"].shape
    keep = torch.from_numpy(np.asarray(out["completion_mask"]).astype(bool)).to(DEV)
    targets = torch.from_numpy(np.asarray(out["completion_ids"]).reshape(-1)).to(DEV)
    lp, _ = eng.pol.logprobs(eng.pol._ws["carry"]["hf"], rows, targets, save=False)
    pol_logp = eng.shadow_policy_head[0]
    assert torch.equal(pol_logp[keep], lp.view(N, Cw)[keep]) and torch.equal(out["logps"][keep], lp.view(N, Cw)[keep])
    eng.pol.logp_temperature = 1.0
    try:
        lp1, _ = eng.pol.logprobs(eng.pol._ws["carry"]["hf"], rows, targets, save=False)
    finally:
        eng.pol.logp_temperature = T
    assert float((lp1.view(N, Cw) - pol_logp)[keep].abs().max()) > 1e-3
