"""trl's sync_ref_model / ref_model_mixup_alpha / ref_model_sync_steps (the TR-DPO reference update) through GRPOArgs / SCGRPOEngine.optimizer_step,
ParamStore.mix_from, GRPOConfig / SCGRPOTrainer (metrics, checkpoints, resume) and the flags of train/stage_rl/grpo_ad.py.  The kernel's own tests are
tests/test_ref_mix.py; its restatement is imported from there."""
import dataclasses
import importlib.util
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fixture_util as fx  # noqa: E402
import iadr1_amd  # noqa: E402,F401
import test_grpo_clip as tgc  # noqa: E402  (_trainer, _row: the TINY trainer with a stub processor)
import test_ref_mix as trm  # noqa: E402  (restate, depth, bits)
import test_rollout_is as tri  # noqa: E402  (stores, tiny_batch, reward_fn: the TINY engine fixtures)
from iadr1_amd import hip  # noqa: E402
from iadr1_amd.params import ParamStore, VLMConfig  # noqa: E402
from iadr1_amd.sc_grpo import GRPOArgs, SCGRPOEngine, check_sync_ref_args, ref_sync_due  # noqa: E402

DEV = "cuda"
CFG = tri.CFG
ALPHA = 0.6
KEYS = ("ref/policy_dist", "ref/syncs")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _grpo_ad():
    spec = importlib.util.spec_from_file_location("grpo_ad_sync_ref_flags", os.path.join(ROOT, "train", "stage_rl", "grpo_ad.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- without a GPU ---------------------------------------------------------------------------------------------------------------------------------------

def test_defaults_are_trl_s():
    from iadr1_amd.trainer import GRPOConfig
    for cls in (GRPOConfig, GRPOArgs):
        d = cls()
        assert d.sync_ref_model is False and d.ref_model_mixup_alpha == 0.6 and d.ref_model_sync_steps == 512, cls


def test_flags_parse_and_the_yaml_path_sets_them(tmp_path):
    from iadr1_amd.trainer import GRPOConfig
    mod = _grpo_ad()
    base = ["--model_name_or_path", "/m", "--output_dir", "o", "--dataset_name", "d.json"]
    d = mod.build_parser().parse_args(base)
    assert d.sync_ref_model is False and d.ref_model_mixup_alpha == 0.6 and d.ref_model_sync_steps == 512
    a = mod.build_parser().parse_args(base + ["--sync_ref_model", "--ref_model_mixup_alpha", "0.25", "--ref_model_sync_steps", "64"])
    assert a.sync_ref_model is True and a.ref_model_mixup_alpha == 0.25 and a.ref_model_sync_steps == 64
    assert mod.build_parser().parse_args(base + ["--sync_ref_model", "true"]).sync_ref_model is True
    assert mod.build_parser().parse_args(base + ["--sync_ref_model", "false"]).sync_ref_model is False
    y = tmp_path / "run.yaml"
    y.write_text("model_name_or_path: /m\noutput_dir: o\ndataset_name: d.json\nsync_ref_model: true\nref_model_mixup_alpha: 0.9\nref_model_sync_steps: 7\n")
    c = mod.parse_args_and_config(mod.build_parser(), ["--config", str(y)])
    assert c.sync_ref_model is True and c.ref_model_mixup_alpha == 0.9 and c.ref_model_sync_steps == 7
    c = mod.parse_args_and_config(mod.build_parser(), ["--config", str(y), "--ref_model_sync_steps", "9"])       # the command line wins
    assert c.ref_model_sync_steps == 9 and c.sync_ref_model is True
    assert {"sync_ref_model", "ref_model_mixup_alpha", "ref_model_sync_steps"} <= set(GRPOConfig.__dataclass_fields__)      # grpo_ad.main copies every parsed flag that is a GRPOConfig field


BAD = [({"beta": 0.0}, "sync_ref_model"),
       ({"ref_model_mixup_alpha": 0.0}, "ref_model_mixup_alpha"), ({"ref_model_mixup_alpha": -0.1}, "ref_model_mixup_alpha"), ({"ref_model_mixup_alpha": 1.5}, "ref_model_mixup_alpha"),
       ({"ref_model_mixup_alpha": float("nan")}, "ref_model_mixup_alpha"), ({"ref_model_mixup_alpha": float("inf")}, "ref_model_mixup_alpha"),
       ({"ref_model_sync_steps": 0}, "ref_model_sync_steps"), ({"ref_model_sync_steps": -4}, "ref_model_sync_steps"), ({"ref_model_sync_steps": 2.0}, "ref_model_sync_steps"),
       ({"ref_model_sync_steps": True}, "ref_model_sync_steps")]


@pytest.mark.parametrize("kw,field", BAD)
def test_bad_values_are_refused_by_name_when_the_engine_or_the_trainer_is_built(kw, field):
    from iadr1_amd.trainer import GRPOConfig, SCGRPOTrainer
    with pytest.raises(ValueError, match=field):
        SCGRPOEngine(None, None, None, GRPOArgs(sync_ref_model=True, **kw))
    with pytest.raises(ValueError, match=field):
        SCGRPOTrainer((CFG, None), [], processing_class=object(), args=GRPOConfig(sync_ref_model=True, **kw))


def test_the_other_two_fields_are_ignored_while_the_option_is_off():
    from iadr1_amd.trainer import GRPOConfig
    assert check_sync_ref_args("GRPOArgs", False, 7.0, 0, 0.0) is None and check_sync_ref_args("GRPOConfig", False, float("nan"), -1, 0.04) is None
    assert check_sync_ref_args("GRPOArgs", True, 1.0, 1, 0.04) is None        # alpha = 1 (a copy) and every step are legal
    GRPOConfig(ref_model_mixup_alpha=7.0, ref_model_sync_steps=0), GRPOArgs(ref_model_mixup_alpha=7.0, ref_model_sync_steps=0)


def test_which_steps_sync():
    """trl's on_step_end rule on the step counter after its increment."""
    assert [s for s in range(1, 11) if ref_sync_due(s, 1)] == list(range(1, 11))
    assert [s for s in range(1, 11) if ref_sync_due(s, 3)] == [3, 6, 9]


def test_resume_without_the_reference_file_is_refused(tmp_path):
    """A checkpoint directory that holds only trainer_state.json + optimizer.safetensors: with the option on the run would continue against the base model."""
    from safetensors.torch import save_file

    from iadr1_amd.trainer import GRPOConfig, SCGRPOTrainer
    ck = tmp_path / "out" / "checkpoint-2"
    ck.mkdir(parents=True)
    (ck / "trainer_state.json").write_text(json.dumps({"global_step": 2, "opt_step": 2, "layout": "x", "n_total": 64}))
    save_file({"master": torch.zeros(64)}, str(ck / "optimizer.safetensors"))
    tr = SCGRPOTrainer.__new__(SCGRPOTrainer)       # no model is needed up to the refusal
    tr.args = GRPOConfig(output_dir=str(tmp_path / "out"), sync_ref_model=True)
    tr._prefetcher = None
    for how in (str(ck), True):
        with pytest.raises(ValueError, match="reference.safetensors"):
            tr.train(resume_from_checkpoint=how)


def test_mix_from_refuses_another_layout():
    a, b = ParamStore(CFG, "cpu", trainable=False), ParamStore(VLMConfig.from_dict(fx.TINY7), "cpu", trainable=False)
    assert a.layout_digest() == ParamStore(CFG, "cpu", trainable=False).layout_digest() != b.layout_digest()
    with pytest.raises(ValueError, match="layout"):
        a.mix_from(b, 0.6)


# ---- GPU, the TINY model ---------------------------------------------------------------------------------------------------------------------------------

def _engine(pol=None, ref=None, **kw):
    if pol is None:
        pol, ref = tri.stores()
    args = dict(num_generations=4, max_prompt_length=4096, max_completion_length=16, seed=5, learning_rate=1e-3)      # 1e-3: one AdamW step moves the bf16 weights
    args.update(kw)
    return SCGRPOEngine(CFG, pol, ref, GRPOArgs(**args)), pol, ref


def _step(eng):
    m = eng.step(tri.tiny_batch(), tri.reward_fn)        # (with its optimizer step: the metrics are read after it)
    torch.cuda.synchronize()
    return m


def _dist64(pol_flat, ref_flat):
    p, r = pol_flat.double().cpu(), ref_flat.double().cpu()
    return math.sqrt(float(((p - r) ** 2).sum() / (r ** 2).sum()))


@pytest.mark.gpu
def test_three_steps_move_the_reference_as_the_restatement_says():
    """(1) ref_model_sync_steps 1, alpha 0.6: after every optimizer step ref.flat is the restatement of (the reference before the step, pol.flat after it), bit for
    bit; ref/policy_dist and ref/syncs on every step, the distance against float64 at the bound of the kernel's sums (each within D * 2^-23, so their ratio's
    square root within D * 2^-23 to first order; 1.001 x for the second order); the step after a sync logs the kl bits of a fresh engine whose reference store was
    loaded with the mixed buffer by hand.  With ref_model_sync_steps 2 the reference moves after step 2 only, and only that step logs the two keys."""
    eng, pol, ref = _engine(sync_ref_model=True, ref_model_mixup_alpha=ALPHA, ref_model_sync_steps=1)
    D = trm.depth(ref.n_total)
    snap = None
    for step in (1, 2, 3):
        before = ref.flat.clone()
        m = _step(eng)
        want = trm.restate(before.cpu(), pol.flat.cpu(), ALPHA)
        assert torch.equal(trm.bits(ref.flat.cpu()), trm.bits(want)), f"step {step}: {int((trm.bits(ref.flat.cpu()) != trm.bits(want)).sum())} elements off the restatement"
        assert not torch.equal(trm.bits(ref.flat), trm.bits(before))
        d64 = _dist64(pol.flat, before)
        print(f"[sync_ref_model] step {step}: ref/policy_dist {m['ref/policy_dist']:.6e} (float64 {d64:.6e}), ref/syncs {m['ref/syncs']}, kl {m['kl']:.6e}")
        assert m["ref/syncs"] == step == eng.ref_syncs and abs(m["ref/policy_dist"] - d64) <= 1.001 * D * 2.0 ** -23 * d64
        if step == 1:       # what a fresh engine needs to repeat step 2: the policy after step 1 and the mixed reference
            snap = {k: getattr(pol, k).clone() for k in ("flat", "master", "m", "v")}
            snap["mixed"] = want
        if step == 2:
            kl2 = m["kl"]
    assert kl2 > 0
    pol_b, ref_b = ParamStore(CFG, DEV, trainable=True), ParamStore(CFG, DEV, trainable=False)
    for k in ("flat", "master", "m", "v"):
        getattr(pol_b, k).copy_(snap[k])
    pol_b.refresh_shadows()
    ref_b.flat.copy_(snap["mixed"])          # by hand: the restatement's buffer, not the kernel's
    ref_b.finalize()
    eng_b, _, _ = _engine(pol_b, ref_b)
    eng_b.opt_step = 1                       # (the rollout's seed derives from it)
    m_b = eng_b.step(tri.tiny_batch(), tri.reward_fn, do_optimizer_step=False)
    torch.cuda.synchronize()
    assert not eng.last_step_shadowed and not eng_b.last_step_shadowed       # both took the sequential step
    assert m_b["kl"] == kl2 and not any(k in m_b for k in KEYS), (m_b["kl"], kl2)
    # every second step
    eng, pol, ref = _engine(sync_ref_model=True, ref_model_mixup_alpha=ALPHA, ref_model_sync_steps=2)
    start = ref.flat.clone()
    m1 = _step(eng)
    assert torch.equal(trm.bits(ref.flat), trm.bits(start)) and not any(k in m1 for k in KEYS) and eng.ref_syncs == 0
    m2 = _step(eng)
    assert torch.equal(trm.bits(ref.flat.cpu()), trm.bits(trm.restate(start.cpu(), pol.flat.cpu(), ALPHA))) and m2["ref/syncs"] == 1 and m2["ref/policy_dist"] > 0


@pytest.mark.gpu
def test_the_moved_reference_is_the_same_co_scheduled_and_sequential(monkeypatch):
    """(2) Two steps with ref_model_sync_steps 1 at 64 sequences, once with the reference's pass on a 64-CU side stream under the rollout and once sequential, set up
    like test_hip_model.test_chunked_reference_pass_is_bit_equal_to_the_one_shot_pass (3B widths, 2 layers, IADR1_DECODE_KS pinned): the per-token reference
    log-probs and the kl of step 2 have equal bits -- the existing equality, now with a reference that moved between the steps (the mix is ordered ahead of the side
    stream's first read of it).  learning_rate 0: the co-scheduled step's GRADIENTS differ from the sequential one's in the last bf16 bit of the rebuilt mlp rows
    (overlap.py), so with a live optimizer the two policies, hence step 2's tokens, would differ for a reason that has nothing to do with the reference; AdamW still
    rewrites pol.flat, with the values it had, and the policy is far from the reference (independent initialisation), so the mix moves every element."""
    cfg = dataclasses.replace(VLMConfig.qwen25vl_3b(), num_hidden_layers=2, v_depth=2, v_fullatt=(1,))
    import test_hip_model as thm
    G, C, Bp = 8, 64, 8
    cd = thm._oracle_cfg_dict(cfg)
    grids = [(1, 16, 16), (1, 16, 12)] * 4
    ids, mask = fx.left_pad([fx.synth_prompt(grids[k], 21 + 3 * k, cd, 5 + k) for k in range(Bp)], cfg.pad_token_id)
    batch = {"input_ids": ids, "attention_mask": mask, "pixel_values": fx.synth_pixel_values(grids, cd, seed=5), "image_grid_thw": grids}
    monkeypatch.setenv("IADR1_DECODE_KS", "1,8")
    res = {}
    for mode in ("64", "0"):
        monkeypatch.setenv("IADR1_OVERLAP_CUS", mode)
        ref = ParamStore(cfg, DEV, trainable=False)
        ref.init_random(seed=0)
        pol = ParamStore(cfg, DEV, trainable=True)
        pol.init_random(seed=1)
        start = ref.flat.clone()
        eng = SCGRPOEngine(cfg, pol, ref, GRPOArgs(num_generations=G, max_prompt_length=4096, max_completion_length=C, micro_batch_seqs=Bp * G, seed=11, beta=0.04, suppress_eos=True,
                                                   learning_rate=0.0, sync_ref_model=True, ref_model_mixup_alpha=ALPHA, ref_model_sync_steps=1))
        try:
            m1 = eng.step(batch, tri.reward_fn)
        except RuntimeError as exc:
            if mode != "0" and "no stream pair" in str(exc):
                pytest.skip(f"co-scheduled case NOT RUN on this box: {exc}")
            raise
        moved = ref.flat.clone()
        out = eng.step(batch, tri.reward_fn, do_optimizer_step=False, return_outputs=True)
        torch.cuda.synchronize()
        assert eng.last_step_shadowed == (mode != "0") and m1["ref/syncs"] == 1 and not torch.equal(trm.bits(moved), trm.bits(start))
        res[mode] = (out, moved.cpu(), m1)
        del eng, pol, ref
    (o1, r1, a1), (o0, r0, a0) = res["64"], res["0"]
    assert torch.equal(trm.bits(r1), trm.bits(r0)) and a1["ref/policy_dist"] == a0["ref/policy_dist"]
    assert np.array_equal(o1["completion_ids"], o0["completion_ids"])
    assert torch.equal(o1["ref_logps"], o0["ref_logps"]) and bool(torch.isfinite(o1["ref_logps"]).all())
    assert torch.equal(o1["kl"], o0["kl"]) and o1["metrics"]["kl"] == o0["metrics"]["kl"] > 0


def _sync_trainer(tmp_path, name, **cfg):
    calls = {"rewards": 0, "ref_forward": 0}
    return tgc._trainer(tmp_path / name, calls, gradient_accumulation_steps=1, logging_steps=1, train_dataset=[tgc._row(0), tgc._row(1), tgc._row(2)], shuffle=False, **cfg)


@pytest.mark.gpu
def test_checkpoint_round_trip(tmp_path):
    """(3) sync on, save_steps 2: checkpoint-2 holds reference.safetensors and ref_syncs; a fresh trainer resumed from it has the reference's bits and the count
    the first run had at that point, and its step 3 logs the kl bits of the uninterrupted run.  A checkpoint of another layout's reference is refused."""
    from iadr1_amd.trainer import REFERENCE_FILE, load_reference_state
    on = dict(sync_ref_model=True, ref_model_mixup_alpha=ALPHA, ref_model_sync_steps=1, save_steps=2, max_steps=3)
    a = _sync_trainer(tmp_path, "a", **on)
    at_save = {}
    save_model = a.save_model

    def saving(path=None):
        at_save.update(flat=a.ref.flat.clone(), syncs=a.engine.ref_syncs)
        return save_model(path)
    a.save_model = saving
    hist = a.train()
    ck = os.path.join(a.args.output_dir, "checkpoint-2")
    assert os.path.exists(os.path.join(ck, REFERENCE_FILE)) and json.load(open(os.path.join(ck, "trainer_state.json")))["ref_syncs"] == 2 == at_save["syncs"]
    assert os.path.getsize(os.path.join(ck, REFERENCE_FILE)) >= 2 * a.ref.n_total
    assert [h["ref/syncs"] for h in hist] == [1, 2, 3] and all(h["ref/policy_dist"] > 0 for h in hist) and hist[2]["kl"] > 0
    b = _sync_trainer(tmp_path, "b", **on)
    base = b.ref.flat.clone()           # the starting checkpoint: what a resume without the file would have left in place
    at_resume = {}
    training_step = b.training_step

    def stepping(*args, **kw):
        if not at_resume:
            at_resume.update(flat=b.ref.flat.clone(), syncs=b.engine.ref_syncs)
        return training_step(*args, **kw)
    b.training_step = stepping
    hist_b = b.train(resume_from_checkpoint=ck)
    assert torch.equal(trm.bits(at_resume["flat"]), trm.bits(at_save["flat"])) and at_resume["syncs"] == 2
    assert not torch.equal(trm.bits(at_save["flat"]), trm.bits(base))
    assert len(hist_b) == 1 and hist_b[0]["step"] == 3 and hist_b[0]["kl"] == hist[2]["kl"] and hist_b[0]["ref/syncs"] == 3 and hist_b[0]["ref/policy_dist"] == hist[2]["ref/policy_dist"]
    other = ParamStore(VLMConfig.from_dict(fx.TINY7), "cpu", trainable=False)
    with pytest.raises(ValueError, match="layout"):
        load_reference_state(other, ck)


@pytest.mark.gpu
def test_option_off_changes_nothing(tmp_path, monkeypatch):
    """(4) no reference.safetensors is written, no ref/* key is logged, hip.call is never reached with ref_mix -- and a checkpoint that HAS the file resumes with the
    option off, against the starting checkpoint as always."""
    from iadr1_amd.trainer import REFERENCE_FILE, save_reference_state
    names = []
    real = hip.call

    def recording(name, *args):
        names.append(name)
        return real(name, *args)
    monkeypatch.setattr(hip, "call", recording)
    t = _sync_trainer(tmp_path, "off", save_steps=2, max_steps=2, ref_model_mixup_alpha=0.9, ref_model_sync_steps=1)
    start = t.ref.flat.clone()
    hist = t.train()
    ck = os.path.join(t.args.output_dir, "checkpoint-2")
    assert os.path.exists(os.path.join(ck, "optimizer.safetensors")) and not os.path.exists(os.path.join(ck, REFERENCE_FILE))
    assert "ref_syncs" not in json.load(open(os.path.join(ck, "trainer_state.json")))
    assert len(hist) == 2 and not any(k.startswith("ref/") for h in hist for k in h)
    assert "adamw_flat" in names and "ref_mix" not in names and torch.equal(trm.bits(t.ref.flat), trm.bits(start))
    save_reference_state(t.policy, ck)          # some file of the right layout: it must not be read
    t2 = _sync_trainer(tmp_path, "off2", save_steps=0, max_steps=3)
    hist2 = t2.train(resume_from_checkpoint=ck)
    assert len(hist2) == 1 and hist2[0]["step"] == 3 and torch.equal(trm.bits(t2.ref.flat), trm.bits(start)) and "ref_mix" not in names
