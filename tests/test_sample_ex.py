"""iadr1_sample_ex / iadr1_seen_init (csrc/sample.hip): trl's GRPOConfig(repetition_penalty, min_p) in the rollout's sampler, and the rollout / engine / entry-point
layers above them.  Filter order as in transformers: repetition penalty -> temperature -> top-k -> top-p -> min_p.  The expectations are numpy: the penalty in
float32 (one IEEE multiply or divide, the kernel's own bits), everything behind it in float64; `restate` is pinned to transformers' processors and warpers
without a GPU.  The oracle contributes its Philox uniforms only.  Inputs are generated on the CPU, so the conditions the GPU cases rely on are asserted there too."""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

import iadr1_amd  # noqa: F401
from iadr1_amd import hip, ops

DEV = "cuda"
F32 = torch.float32
VOCABS = [640, 20011, 151936]      # per = 1 (most threads idle); prime: csize 626, per 3, chunk starts and thread slices straddle bitmap words; the real row, per 19
B, T, MIN_P, PEN, SEED = 8, 0.9, 0.05, 1.3, 1
# top_k = 50, top_p = 0.9: a min_p at which, on these inputs, the min_p prefix is the shorter in some rows and the top-p prefix in others (asserted without a GPU).
# V = 640 has 50 candidates among 640 tokens, not among thousands: its top-50 weights fall off faster, at 0.2 min_p would be the shorter prefix in every row
MIN_P_TOPK = {640: 0.06, 20011: 0.2, 151936: 0.2}
SENT = 0x5A5A5A5A                   # sentinel words around every bitmap


@functools.lru_cache(maxsize=None)
def inputs(V):
    """(logits [B, V] float32, seen ids [B, 203] int64): randn * 2.5 and, per row, 200 ids from randint of the same generator + the row's top-3 ids -- so that the
    penalty moves the row maximum (all 8 rows at the larger V, 5 - 8 of 8 at V = 640 for seeds 1 - 3).  Computed once, never modified."""
    g = torch.Generator().manual_seed(SEED)
    x = (torch.randn(B, V, generator=g) * 2.5).to(F32)
    ids = torch.randint(0, V, (B, 200), generator=g)
    ids = torch.cat([ids, x.topk(3, dim=1).indices], 1)
    return x.numpy(), ids.numpy()


def words(V):
    return (V + 31) // 32


def bitmap(ids, V, ld=None):
    """[rows, ld] uint32 bitmap of the id lists (ids outside [0, V) ignored)."""
    bm = np.zeros((len(ids), ld or words(V)), dtype=np.uint32)
    for r, row in enumerate(ids):
        for t in row:
            if 0 <= int(t) < V:
                bm[r, int(t) >> 5] |= np.uint32(1 << (int(t) & 31))
    return bm


def to_dev(bm):
    return torch.from_numpy(bm.view(np.int32).copy()).to(DEV)


def framed(bm):
    """The bitmap inside a larger allocation, 8 sentinel words in front and behind: returns (whole flat buffer, the [rows, ld] view the kernels get)."""
    rows, ld = bm.shape
    buf = np.full(16 + rows * ld, SENT, dtype=np.uint32)
    buf[8: 8 + rows * ld] = bm.reshape(-1)
    whole = torch.from_numpy(buf.view(np.int32).copy()).to(DEV)
    return whole, whole[8: 8 + rows * ld].view(rows, ld)


def unframed(whole):
    a = whole.cpu().numpy().view(np.uint32)
    assert (a[:8] == SENT).all() and (a[-8:] == SENT).all(), "a write outside the bitmap"
    return a[8:-8]


def penalise32(x, ids, pen):
    """RepetitionPenaltyLogitsProcessor in numpy float32: seen ids get x * pen (x < 0) or x / pen, one rounding each."""
    xp = x.copy()
    p = np.float32(pen)
    for r in range(x.shape[0]):
        u = np.unique(ids[r])
        v = x[r, u]
        xp[r, u] = np.where(v < 0, v * p, v / p).astype(np.float32)
    return xp


def restate(xp_row, temp, top_k, top_p, min_p, sup=-1):
    """float64 restatement of temperature -> top-k -> top-p -> min_p on one (already penalised, float32) row.  Returns (ids, probs, n_topp, n_minp): the kept ids
    in rank order (value descending, id ascending; all of them for top_k <= 0), their renormalised probabilities, and the lengths of the top-p and min_p prefixes."""
    z = xp_row.astype(np.float64) / temp
    if sup >= 0:
        z = z.copy()
        z[sup] = -np.inf
    order = np.lexsort((np.arange(z.size), -z))
    if top_k > 0:
        order = order[: min(top_k, z.size)]
    w = np.exp(z[order] - z[order[0]])
    before = np.concatenate([[0.0], np.cumsum(w)[:-1]])
    n_topp = int(np.sum(before < top_p * w.sum())) if top_p < 1.0 else int(np.sum(w > 0))
    n_minp = int(np.sum(w >= min_p)) if min_p > 0 else int(np.sum(w > 0))
    n = max(1, min(n_topp, n_minp))
    return order[:n], w[:n] / w[:n].sum(), n_topp, n_minp


def kept_cdf(xp_row, temp, min_p, sup):
    """Whole vocabulary: (weights in id order with the dropped and the suppressed ids at 0, their cumulative sum, the undropped weights)."""
    z = xp_row.astype(np.float64)
    m = np.delete(z, sup).max() if sup >= 0 else z.max()
    w_all = np.exp((z - m) / temp)
    if sup >= 0:
        w_all[sup] = 0.0
    w = np.where(w_all >= min_p, w_all, 0.0)
    return w, np.cumsum(w), w_all


def ref_logp(lg, ids):
    return torch.log_softmax(lg.double(), -1).gather(1, ids.view(-1, 1)).squeeze(1)


def close(got, ref, rtol, atol, what=""):
    got, ref = got.double().cpu(), ref.double().cpu()
    err = (got - ref).abs()
    tol = atol + rtol * ref.abs()
    assert not bool((err > tol).any()), f"{what}: {int((err > tol).sum())}/{ref.numel()} out of tol, max|err| {err.max().item():.4g}"


# ---- without a GPU ---------------------------------------------------------------------------------------------------------------------------------------

def test_abi_has_the_two_entry_points():
    L = hip.lib()
    assert hip.version() >= 115
    for name in ("iadr1_sample_ex", "iadr1_sample_ex_workspace_bytes", "iadr1_seen_init"):
        assert name in hip.PROTOS and hasattr(L, name)
    assert L.iadr1_sample_ex_workspace_bytes(64) >= L.iadr1_sample_logp_workspace_bytes(64)


def _ex(L, *, B_=1, V=64, T_=0.9, k=50, p=0.9, min_p=0.0, pen=1.0, seen=None, ld_seen=0, mark=0):
    rc = L.iadr1_sample_ex(None, 0, None, None, 0, 0, None, B_, V, T_, k, p, min_p, pen, seen, ld_seen, mark, -1, 0, 0, None, None, None)
    return rc, L.iadr1_last_error()


def test_host_refusals_each_have_their_own_message_without_a_gpu():
    """Every refusal is detected before any launch (all buffers NULL, no device touched): rc < 0 and a message that names the cause."""
    L = hip.lib()
    msgs = []
    for mp in (1.0, -0.1, 1.5, float("nan")):
        rc, m = _ex(L, min_p=mp)
        assert rc < 0 and b"sample_ex" in m and b"min_p" in m and b"repetition_penalty" not in m, (mp, m)
    msgs.append(m)
    for pen in (0.0, -1.0, float("nan"), float("inf")):
        rc, m = _ex(L, pen=pen)
        assert rc < 0 and b"sample_ex" in m and b"repetition_penalty must be finite" in m, (pen, m)
    msgs.append(m)
    some = 0x1000       # a non-NULL address: refused on ld_seen before anything could read it
    for kw in (dict(pen=1.3), dict(mark=1), dict(pen=1.3, seen=some, ld_seen=1), dict(mark=1, seen=some, ld_seen=1)):
        rc, m = _ex(L, **kw)
        assert rc < 0 and b"sample_ex" in m and b"seen" in m and b"ceil(V / 32)" in m, (kw, m)
    msgs.append(m)
    for k in (0, -1):       # what iadr1_sample_logp refuses
        rc, m = _ex(L, k=k, p=0.9, min_p=0.05)
        assert rc < 0 and b"sample_ex" in m and b"top_p" in m and b"nucleus" in m
    msgs.append(m)
    rc, m = _ex(L, p=0.0)
    assert rc < 0 and b"top_p must be in" in m
    rc, m = _ex(L, B_=0)
    assert rc < 0 and b"empty problem" in m
    assert len(set(msgs)) == len(msgs)
    assert L.iadr1_seen_init(None, 4, None, 1, 1, 64, None, 2, None) < 0 and b"seen_init" in L.iadr1_last_error()


def test_grpo_args_and_entry_point_flags():
    from iadr1_amd.sc_grpo import GRPOArgs, SCGRPOEngine
    from iadr1_amd.trainer import GRPOConfig
    for kw, word in ((dict(min_p=1.0), "min_p"), (dict(min_p=-0.1), "min_p"), (dict(repetition_penalty=0), "repetition_penalty"), (dict(repetition_penalty=float("nan")), "repetition_penalty")):
        with pytest.raises(ValueError, match=word):
            SCGRPOEngine(None, None, None, GRPOArgs(**kw))
    a, c = GRPOArgs(), GRPOConfig()
    assert (a.min_p, a.repetition_penalty, c.min_p, c.repetition_penalty) == (0.0, 1.0, 0.0, 1.0)
    assert GRPOArgs(min_p=None).min_p is None       # trl's None is accepted and means 0 (check_sampler_args)
    from iadr1_amd.sc_grpo import check_sampler_args
    assert check_sampler_args("GRPOArgs", None, 1.0) == 0.0 and check_sampler_args("GRPOConfig", 0.05, 1.3) == 0.05
    m = __import__("importlib").util
    spec = m.spec_from_file_location("grpo_ad_flags_ex", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "train", "stage_rl", "grpo_ad.py"))
    mod = m.module_from_spec(spec)
    spec.loader.exec_module(mod)
    base = ["--model_name_or_path", "/m", "--output_dir", "o", "--dataset_name", "d.json"]
    d = mod.build_parser().parse_args(base)
    assert d.min_p == 0.0 and d.repetition_penalty == 1.0
    s = mod.build_parser().parse_args(base + ["--min_p", "0.05", "--repetition_penalty", "1.2"])
    assert s.min_p == 0.05 and s.repetition_penalty == 1.2


def test_config_file_sets_both_options(tmp_path):
    m = __import__("importlib").util
    spec = m.spec_from_file_location("grpo_ad_flags_ex2", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "train", "stage_rl", "grpo_ad.py"))
    mod = m.module_from_spec(spec)
    spec.loader.exec_module(mod)
    f = tmp_path / "c.yaml"
    f.write_text("model_name_or_path: /m\noutput_dir: o\ndataset_name: d.json\nmin_p: 0.1\nrepetition_penalty: 1.15\n")
    a = mod.parse_args_and_config(mod.build_parser(), ["--config", str(f)])
    assert a.min_p == 0.1 and a.repetition_penalty == 1.15


def test_restatement_equals_the_transformers_processors():
    """The restatement the GPU cases use against transformers on the V = 640 inputs: RepetitionPenaltyLogitsProcessor on the float32 row (bit-equal to penalise32),
    then Temperature -> TopK -> TopP -> MinP warpers in float64: the same kept set, probabilities within 1e-12.  top_k = 50 / top_p = 0.9 with both min_p values,
    and the whole vocabulary (no top-k, no top-p) with min_p."""
    from transformers.generation.logits_process import (MinPLogitsWarper, RepetitionPenaltyLogitsProcessor, TemperatureLogitsWarper, TopKLogitsWarper,
                                                        TopPLogitsWarper)
    x, ids = inputs(640)
    xp = penalise32(x, ids, PEN)
    hf_pen = RepetitionPenaltyLogitsProcessor(PEN)(torch.from_numpy(ids), torch.from_numpy(x.copy()))
    assert hf_pen.dtype == F32 and np.array_equal(hf_pen.numpy().view(np.uint32), xp.view(np.uint32))
    moved = (xp.argmax(1) != x.argmax(1)).sum()
    assert moved >= 5
    for top_k, top_p, min_p in ((50, 0.9, MIN_P), (50, 0.9, MIN_P_TOPK[640]), (50, 0.9, 0.2), (0, 1.0, MIN_P)):
        s = TemperatureLogitsWarper(T)(None, hf_pen.double())
        if top_k > 0:
            s = TopKLogitsWarper(top_k)(None, s)
        if top_p < 1:
            s = TopPLogitsWarper(top_p)(None, s)
        s = MinPLogitsWarper(min_p)(None, s)
        pr = torch.softmax(s, -1).numpy()
        for b in range(B):
            kid, kp, _, _ = restate(xp[b], T, top_k, top_p, min_p)
            assert set(np.flatnonzero(pr[b] > 0).tolist()) == set(kid.tolist()), (top_k, min_p, b)
            assert np.abs(pr[b, kid] - kp).max() < 1e-12
            if top_k <= 0:      # the id-order form the whole-vocabulary cases use is the same distribution
                w, cdf, _ = kept_cdf(xp[b], T, min_p, -1)
                assert np.abs(w / cdf[-1] - pr[b]).max() < 1e-12


@pytest.mark.parametrize("V", VOCABS)
def test_conditions_of_the_gpu_cases_hold_on_these_inputs(V):
    """Conditions, not measurements: (a) no token sits within 1e-4 (relative) of the min_p threshold, in the whole-vocabulary case or among the top-50, and no
    top-p cut sits within 1e-4 of its boundary, so kept-or-dropped is not a rounding question; (b) at MIN_P_TOPK[V] both prefixes are the shorter one somewhere;
    (c) the penalty moves the row maximum (all rows at the larger V)."""
    x, ids = inputs(V)
    xp = penalise32(x, ids, PEN)
    sup = int(xp[5].argmax())
    kept = []
    for s in (-1, sup):
        for b in range(B):
            w, _, w_all = kept_cdf(xp[b], T, MIN_P, s)
            assert not (np.abs(w_all / MIN_P - 1) < 1e-4).any()
            kept.append(int((w > 0).sum()))
    assert min(kept) >= 2 and max(kept) < V // 2
    shorter = set()
    for b in range(B):
        for mp in (MIN_P, MIN_P_TOPK[V]):
            kid, _, n_topp, n_minp = restate(xp[b], T, 50, 0.9, mp)
            z = np.sort(xp[b].astype(np.float64))[::-1][:50] / T
            w = np.exp(z - z[0])
            assert not (np.abs(w / mp - 1) < 1e-4).any()
            before = np.cumsum(w)[:-1]
            assert not (np.abs(before / (0.9 * w.sum()) - 1) < 1e-4).any()
            if mp == MIN_P_TOPK[V] and n_topp != n_minp:
                shorter.add("min_p" if n_minp < n_topp else "top_p")
    assert shorter == {"min_p", "top_p"}
    moved = int((xp.argmax(1) != x.argmax(1)).sum())
    assert moved == B if V > 640 else moved >= 5
    print(f"[sample_ex inputs] V={V}: whole-vocabulary kept per row {min(kept)}..{max(kept)}, maximum moved in {moved}/{B} rows")


# ---- the kernels -----------------------------------------------------------------------------------------------------------------------------------------

def steps_for(V):
    return 20 if V < 100000 else 3


@pytest.mark.gpu
@pytest.mark.parametrize("V", VOCABS)
def test_neutral_settings_are_bit_equal_to_sample_logp(V):
    """(1) min_p 0, penalty 1, mark_seen 0: ids and log-probs bit-equal to ops.sample_logp for top-k 50, the whole vocabulary and greedy, with and without a
    suppressed token, with a garbage-filled seen buffer passed -- which stays as it was, inside its sentinels."""
    x, _ = inputs(V)
    lg = torch.from_numpy(x).to(DEV)
    sup = int(x[5].argmax())
    garbage = np.random.default_rng(3).integers(0, 2 ** 32, size=(B, words(V)), dtype=np.uint64).astype(np.uint32)
    whole, seen = framed(garbage)
    for T_, k, p in ((T, 50, 0.9), (T, 0, 1.0), (0.0, 1, 1.0)):
        for s in (-1, sup):
            for step in range(3):
                for sn in (seen, None):
                    a, la = ops.sample_logp(lg, T_, k, p, seed=77, step=step, suppress_token=s, logp_out=torch.zeros(B, 4, device=DEV))
                    b, lb = ops.sample_ex(lg, T_, k, p, seed=77, step=step, seen=sn, suppress_token=s, logp_out=torch.zeros(B, 4, device=DEV))
                    assert torch.equal(a, b) and torch.equal(la, lb), (T_, k, s, step)
    assert np.array_equal(unframed(whole), garbage.reshape(-1))


@pytest.mark.gpu
@pytest.mark.parametrize("V", VOCABS)
def test_greedy_honours_the_penalty(V):
    """(2) T = 0: the ids are the argmax of the numpy-float32-penalised row (lowest index on ties) -- an equality; min_p is ignored; wherever the penalty moves the
    maximum the id differs from the unpenalised argmax.  A tie made by the penalty itself (two seen copies of the top value) resolves to the lower index."""
    x, ids = inputs(V)
    x = x.copy()
    hi = np.float32(x[3].max() * 2)
    x[3, 5] = x[3, V - 7] = hi          # both seen below: both penalised to the same value, above everything else in the row
    ids = np.concatenate([ids, np.tile(np.array([[5, V - 7]]), (B, 1))], 1)
    xp = penalise32(x, ids, PEN)
    want = xp.argmax(1)
    assert want[3] == 5
    lg, seen = torch.from_numpy(x).to(DEV), to_dev(bitmap(ids, V))
    for k, mp in ((50, 0.0), (0, 0.0), (50, MIN_P), (1, MIN_P)):
        got = ops.sample_ex(lg, 0.0, k, 1.0, seed=1, step=0, min_p=mp, repetition_penalty=PEN, seen=seen, want_logp=False)[0].cpu().numpy()
        assert np.array_equal(got, want), (k, mp, got, want)
    raw = x.argmax(1)
    moved = want != raw
    assert moved.sum() >= 5 and (got[moved] != raw[moved]).all()
    sup = int(want[2])
    xs = xp.copy()
    xs[:, sup] = -np.inf
    got = ops.sample_ex(lg, 0.0, 50, 1.0, seed=1, step=0, repetition_penalty=PEN, seen=seen, suppress_token=sup, want_logp=False)[0].cpu().numpy()
    assert np.array_equal(got, xs.argmax(1))


@pytest.mark.gpu
@pytest.mark.parametrize("V", VOCABS)
def test_whole_vocabulary_with_penalty_and_min_p(V):
    """(3) top_k = 0: every draw against the float64 cumulative weights in id order over the kept set, in the form (and with the tolerance, 1e-4 x total) of
    test_whole_vocabulary_draw_is_the_inverse_cdf_in_id_order: the summation tree is no deeper (the chunk masses are formed in stage 2 with stage 1's tree).  No
    dropped and no suppressed id is ever drawn; two runs are identical; scalar and device-resident step / seed agree.  Kept-or-dropped is not a rounding question
    on these inputs: no token within 1e-4 of the threshold (asserted here and, without a GPU, in test_conditions_of_the_gpu_cases_hold_on_these_inputs)."""
    from oracle import sampler as osamp
    x, ids = inputs(V)
    xp = penalise32(x, ids, PEN)
    lg, seen = torch.from_numpy(x).to(DEV), to_dev(bitmap(ids, V))
    sup = int(xp[5].argmax())
    seed = 1234567890123
    kw = dict(min_p=MIN_P, repetition_penalty=PEN, seen=seen, want_logp=False)
    for s in (-1, sup):
        ref = [kept_cdf(xp[b], T, MIN_P, s) for b in range(B)]
        for w, cdf, w_all in ref:
            assert not (np.abs(w_all / MIN_P - 1) < 1e-4).any()
        for step in range(steps_for(V)):
            got = ops.sample_ex(lg, T, 0, 1.0, seed=seed, step=step, suppress_token=s, **kw)[0]
            assert torch.equal(got, ops.sample_ex(lg, T, 0, 1.0, seed=seed, step=step, suppress_token=s, **kw)[0])
            for b, t in enumerate(got.tolist()):
                w, cdf, _ = ref[b]
                tol = 1e-4 * cdf[-1]
                u = osamp.philox_uniform(seed, b, step) * cdf[-1]
                assert 0 <= t < V and t != s and w[t] > 0, (V, s, step, b, t)
                lo = cdf[t - 1] if t > 0 else 0.0
                assert lo - tol <= u <= cdf[t] + tol, (V, s, step, b, t, lo / cdf[-1], u / cdf[-1], cdf[t] / cdf[-1])
    sp = torch.tensor([7], dtype=torch.int32, device=DEV)
    sd = torch.tensor([seed], dtype=torch.int64, device=DEV)
    want = ops.sample_ex(lg, T, 0, 1.0, seed=seed, step=7, **kw)[0]
    assert torch.equal(ops.sample_ex(lg, T, 0, 1.0, seed=seed, step=0, step_ptr=sp, **kw)[0], want)
    assert torch.equal(ops.sample_ex(lg, T, 0, 1.0, seed=0, step=7, seed_ptr=sd, **kw)[0], want)
    # each option alone: the penalty without min_p keeps every token, min_p without a bitmap reads the raw row
    for mp, pen, rows in ((0.0, PEN, xp), (MIN_P, 1.0, x)):
        got = ops.sample_ex(lg, T, 0, 1.0, seed=seed, step=1, min_p=mp, repetition_penalty=pen, seen=seen if pen != 1 else None, want_logp=False)[0].tolist()
        for b, t in enumerate(got):
            w, cdf, _ = kept_cdf(rows[b], T, mp, -1)
            u = osamp.philox_uniform(seed, b, 1) * cdf[-1]
            assert w[t] > 0 and (cdf[t - 1] if t > 0 else 0.0) - 1e-4 * cdf[-1] <= u <= cdf[t] + 1e-4 * cdf[-1], (mp, pen, b, t)


@pytest.mark.gpu
@pytest.mark.parametrize("V", VOCABS)
def test_top_k_path_with_penalty_and_min_p(V):
    """(4) top_k = 50, top_p = 0.9: the candidates are the top-50 of the PENALISED row, the kept prefix is the shorter of the top-p and the min_p prefix of the
    float64 restatement, and every draw lies on the float64 CDF in rank order within 1e-4 x total.  At MIN_P_TOPK[V] both prefixes are the shorter one in some row."""
    from oracle import sampler as osamp
    x, ids = inputs(V)
    xp = penalise32(x, ids, PEN)
    lg, seen = torch.from_numpy(x).to(DEV), to_dev(bitmap(ids, V))
    seed = 424242
    which = set()
    for mp in (MIN_P_TOPK[V], MIN_P):
        ref = [restate(xp[b], T, 50, 0.9, mp) for b in range(B)]
        raw_top = [set(np.argsort(-x[b].astype(np.float64), kind="stable")[:50].tolist()) for b in range(B)]
        assert any(not set(r[0].tolist()) <= raw_top[b] or r[0][0] != x[b].argmax() for b, r in enumerate(ref))     # the raw row would give another answer
        if mp == MIN_P_TOPK[V]:
            which = {("min_p" if r[3] < r[2] else "top_p") for r in ref if r[2] != r[3]}
        for step in range(steps_for(V)):
            got = ops.sample_ex(lg, T, 50, 0.9, seed=seed, step=step, min_p=mp, repetition_penalty=PEN, seen=seen, want_logp=False)[0].tolist()
            for b, t in enumerate(got):
                kid, kp, _, _ = ref[b]
                pos = np.flatnonzero(kid == t)
                assert pos.size == 1, (V, mp, step, b, t, kid)
                j = int(pos[0])
                cdf = np.cumsum(kp)
                u = osamp.philox_uniform(seed, b, step)
                assert (cdf[j - 1] if j else 0.0) - 1e-4 <= u <= cdf[j] + 1e-4, (V, mp, step, b, t, j, u)
    assert which == {"min_p", "top_p"}


@pytest.mark.gpu
@pytest.mark.parametrize("V", VOCABS)
def test_logp_stays_the_raw_row_log_softmax(V):
    """(5) With penalty and min_p on, logp_out is the float64 log-softmax of the RAW row at the pick, at test_logp_is_the_full_row_log_softmax_of_the_pick's bound
    (1e-5, 1e-5): top-k, whole vocabulary, greedy, with a suppressed token (which still counts in the normaliser)."""
    x, ids = inputs(V)
    lg, seen = torch.from_numpy(x).to(DEV), to_dev(bitmap(ids, V))
    sup = int(x[5].argmax())
    for T_, k, p, s in ((T, 50, 0.9, -1), (T, 50, 0.9, sup), (T, 0, 1.0, -1), (T, 0, 1.0, sup), (0.0, 50, 0.9, -1), (0.0, 0, 1.0, sup)):
        got, lp = ops.sample_ex(lg, T_, k, p, seed=99, step=0, min_p=MIN_P, repetition_penalty=PEN, seen=seen, suppress_token=s)
        assert lp.shape == (B, 1) and (s < 0 or got[5].item() != sup)
        close(lp[:, 0], ref_logp(lg, got), 1e-5, 1e-5, f"logp T={T_} k={k} suppress={s}")
    buf = torch.full((B, 6), 7.0, device=DEV)
    sp = torch.tensor([4], dtype=torch.int32, device=DEV)
    got, _ = ops.sample_ex(lg, T, 0, 1.0, seed=3, step=0, step_ptr=sp, min_p=MIN_P, repetition_penalty=PEN, seen=seen, logp_out=buf)
    close(buf[:, 4], ref_logp(lg, got), 1e-5, 1e-5, "column from step_ptr")
    assert bool((buf[:, [0, 1, 2, 3, 5]] == 7.0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("V", VOCABS)
def test_mark_seen_sets_exactly_the_picks(V):
    """(6) After one call with mark_seen the bitmap is the old one OR the picks' bits, word for word, for the three paths; with mark_seen off it is unchanged.  The
    marked token is penalised by the next call: greedy then moves on to another id in every row."""
    x, ids = inputs(V)
    lg = torch.from_numpy(x).to(DEV)
    bm = bitmap(ids, V)
    for T_, k, p in ((T, 50, 0.9), (T, 0, 1.0), (0.0, 1, 1.0)):
        whole, seen = framed(bm)
        got = ops.sample_ex(lg, T_, k, p, seed=5, step=2, min_p=MIN_P, repetition_penalty=PEN, seen=seen, mark_seen=False, want_logp=False)[0]
        assert np.array_equal(unframed(whole), bm.reshape(-1))
        got2 = ops.sample_ex(lg, T_, k, p, seed=5, step=2, min_p=MIN_P, repetition_penalty=PEN, seen=seen, mark_seen=True, want_logp=False)[0]
        assert torch.equal(got, got2)
        want = bm.copy()
        for b, t in enumerate(got.tolist()):
            want[b, t >> 5] |= np.uint32(1 << (t & 31))
        assert np.array_equal(unframed(whole), want.reshape(-1)), (T_, k)
    # mark_seen alone (penalty 1, min_p 0): the sample_logp ids, and their bits
    whole, seen = framed(np.zeros_like(bm))
    a = ops.sample_logp(lg, T, 50, 0.9, seed=5, step=2, want_logp=False)[0]
    b_ = ops.sample_ex(lg, T, 50, 0.9, seed=5, step=2, seen=seen, mark_seen=True, want_logp=False)[0]
    assert torch.equal(a, b_) and np.array_equal(unframed(whole), bitmap([[t] for t in a.tolist()], V).reshape(-1))
    # greedy chain from an empty bitmap: every step's argmax was marked by the step before, so with a strong penalty the ids of consecutive steps differ
    whole, seen = framed(np.zeros_like(bm))
    first = ops.sample_ex(lg, 0.0, 1, 1.0, seed=0, step=0, repetition_penalty=PEN, seen=seen, mark_seen=True, want_logp=False)[0].cpu().numpy()
    second = ops.sample_ex(lg, 0.0, 1, 1.0, seed=0, step=1, repetition_penalty=PEN, seen=seen, mark_seen=True, want_logp=False)[0].cpu().numpy()
    assert np.array_equal(first, x.argmax(1)) and np.array_equal(second, penalise32(x, first[:, None], PEN).argmax(1))


@pytest.mark.gpu
def test_seen_init_from_a_ragged_left_padded_batch():
    """(6) ops.seen_init: ragged left-padded prompts, G = 3, one id >= V and one negative id in live columns (ignored), ids >= V in the padding (not read): exactly
    the expected bitmap, stale contents gone, the rows beyond Bp * G and the sentinels around the buffer intact."""
    V, S, G = 20011, 37, 3
    rng = np.random.default_rng(4)
    lengths = np.array([37, 1, 20, 0, 9], dtype=np.int32)
    Bp = len(lengths)
    ids = np.full((Bp, S), V + 5, dtype=np.int64)            # left padding holds an id that would be out of bounds if it were read
    live = []
    for b, n in enumerate(lengths):
        row = rng.integers(0, V, size=n)
        if b == 0:
            row[3], row[4], row[5], row[6] = V, -1, V - 1, 0      # ignored, ignored, the last id, the first id
            row[7] = row[8] = 12345                               # a repeated id
        ids[b, S - n:] = row
        live.append(row)
    ld = words(V) + 3
    stale = np.random.default_rng(5).integers(0, 2 ** 32, size=(Bp * G + 2, ld), dtype=np.uint64).astype(np.uint32)
    whole, seen = framed(stale)
    ops.seen_init(torch.from_numpy(ids).to(DEV), torch.from_numpy(lengths).to(DEV), G, V, seen[: Bp * G])
    want = stale.copy()
    want[: Bp * G] = bitmap([live[r // G] for r in range(Bp * G)], V, ld)
    assert np.array_equal(unframed(whole), want.reshape(-1))
    assert want[0, (V - 1) >> 5] >> ((V - 1) & 31) & 1 and want[0, 0] & 1 and (want[9:12] == 0).all()


@pytest.mark.gpu
def test_frequencies_with_penalty_and_min_p():
    """(7) In the form of test_whole_vocabulary_frequencies: row 0 of the V = 640 inputs with its seen set, 64 rows x 160 steps = 10 240 whole-vocabulary draws at
    T = 0.9, penalty 1.3, min_p 0.05 against float64 softmax(x' / T) restricted to the kept set.  Over the tokens with expected count >= 5: every one drawn,
    |count - N p| < 4 sigma, chi-square < (n - 1) + 4.5 sqrt(2 (n - 1)) + 4; no dropped token is ever drawn.  An exact float64 inverse-CDF sampler on the same
    Philox uniforms (oracle.sampler.philox_uniform) gives, for sampler seed 979, max 2.77 sigma and chi-square 29.2 against 75.1 (35 tokens kept, all 35 tested);
    seeds 1, 2, 3 and 7 sit inside both bounds too (2.26 / 48.6, 3.02 / 36.3, 3.06 / 52.9, 2.23 / 29.2)."""
    x, ids = inputs(640)
    R, STEPS = 64, 160
    N = R * STEPS
    xp = penalise32(x[:1], ids[:1], PEN)[0]
    w, cdf, _ = kept_cdf(xp, T, MIN_P, -1)
    pr = w / cdf[-1]
    lg = torch.from_numpy(x[0]).to(DEV).repeat(R, 1).contiguous()
    seen = to_dev(np.repeat(bitmap(ids[:1], 640), R, 0))
    draws = torch.stack([ops.sample_ex(lg, T, 0, 1.0, seed=979, step=s, min_p=MIN_P, repetition_penalty=PEN, seen=seen, want_logp=False)[0] for s in range(STEPS)]).flatten().cpu().numpy()
    cnt = np.bincount(draws, minlength=640).astype(np.float64)
    assert cnt[pr == 0].sum() == 0, "a dropped token was drawn"
    sel = N * pr >= 5
    n = int(sel.sum())
    assert n > 20
    z = np.abs(cnt - N * pr)[sel] / np.sqrt(N * pr * (1 - pr))[sel]
    chi2 = float((((cnt - N * pr) ** 2) / np.where(sel, N * pr, 1.0))[sel].sum())
    print(f"[sample_ex frequencies] {n} tokens tested, max {z.max():.2f} sigma, chi2 {chi2:.1f} for {n - 1} dof")
    assert (cnt[sel] > 0).all(), "a token with expected count >= 5 is never drawn"
    assert z.max() < 4.0, f"frequency off by {z.max():.2f} sigma"
    assert chi2 < (n - 1) + 4.5 * math.sqrt(2 * (n - 1)) + 4, f"chi2 {chi2:.1f} for {n - 1} dof"



# ---- rollout and engine (the TINY fixture model of tests/test_rollout_logps.py) --------------------------------------------------------------------------

def _tiny():
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import fixture_util as fx
    from iadr1_amd.params import ParamStore, VLMConfig
    cfg = VLMConfig.from_dict(fx.TINY)
    w = fx.make_weights(fx.TINY, 0)
    pol, ref = ParamStore(cfg, DEV, trainable=True), ParamStore(cfg, DEV, trainable=False)
    pol.load_named(w)
    ref.load_named(w)
    grids = [(1, 16, 12), (1, 8, 8)]
    rows = [fx.synth_prompt(gr, n, fx.TINY, 77 + i) for i, (gr, n) in enumerate(zip(grids, [5, 17]))]
    ids, mask = fx.left_pad(rows, fx.TINY["pad_token_id"])
    batch = {"input_ids": ids, "attention_mask": mask, "pixel_values": fx.synth_pixel_values(grids, fx.TINY, seed=77), "image_grid_thw": grids}
    return cfg, pol, ref, batch


G_TINY, C_TINY = 4, 16


def _rollout_of(use_graph=True, **kw):
    """(engine, its Rollout, plan, image embeddings, batch): one default rollout through the engine builds the pool (and, with use_graph, captures the default step)."""
    from iadr1_amd.sc_grpo import GRPOArgs, SCGRPOEngine
    cfg, pol, ref, batch = _tiny()
    eng = SCGRPOEngine(cfg, pol, ref, GRPOArgs(num_generations=G_TINY, max_prompt_length=4096, max_completion_length=C_TINY, seed=5, use_hip_graph=use_graph, **kw))
    eng.rollout(batch)
    vis = eng.vision_policy(batch, save=False)
    gpr, off = eng._per_row_images(batch, vis["grids"], vis["rows"])
    plan = eng.pol.text_plan(np.asarray(batch["input_ids"]), np.asarray(batch["attention_mask"]), gpr, off)
    return eng, eng._rollout, plan, vis["img"], batch


@pytest.mark.gpu
def test_rollout_graph_and_eager_give_the_same_ids():
    """generate(min_p=0.05, repetition_penalty=1.3): identical ids from the captured graph and from eager launches, and again on a second call with the same seed
    (the bitmap is rebuilt from the prompts by every call, the capture's two extra steps leave no mark); the options change what is sampled."""
    got = {}
    for use_graph in (True, False):
        _, r, plan, img, _ = _rollout_of(use_graph)
        plain = r.generate(plan, img, G_TINY, C_TINY, seed=9).cpu().numpy()
        a = r.generate(plan, img, G_TINY, C_TINY, seed=9, min_p=MIN_P, repetition_penalty=PEN).cpu().numpy()
        assert (r.graph is not None) == use_graph and r.seen is not None
        b = r.generate(plan, img, G_TINY, C_TINY, seed=9, min_p=MIN_P, repetition_penalty=PEN).cpu().numpy()
        assert np.array_equal(a, b) and not np.array_equal(a, plain)
        assert np.array_equal(plain, r.generate(plan, img, G_TINY, C_TINY, seed=9).cpu().numpy())      # and back
        got[use_graph] = a
    assert np.array_equal(got[True], got[False])


@pytest.mark.gpu
def test_bitmap_after_a_rollout_is_prompt_plus_outputs():
    """suppress_eos (no row finishes): after the call rollout.seen is exactly {live prompt tokens of the row's prompt, image placeholders included} | {the row's
    max_new output tokens} -- for the call that captured the graph (the warm-up's and the capture's marks are restored away) and for the next one (the bitmap is
    re-initialised per call)."""
    _, r, plan, img, batch = _rollout_of(True)
    V = r.e.cfg.vocab_size
    ids, mask = np.asarray(batch["input_ids"]), np.asarray(batch["attention_mask"])
    prompt = [ids[b][mask[b] != 0].tolist() for b in range(ids.shape[0])]
    for call, seed in enumerate((21, 22)):
        graph_before = r.graph
        toks = r.generate(plan, img, G_TINY, C_TINY, seed=seed, suppress_eos=True, min_p=MIN_P, repetition_penalty=PEN).cpu().numpy()
        assert (r.graph is not graph_before) == (call == 0), "the first call captures, the second replays"
        assert toks.shape == (ids.shape[0] * G_TINY, C_TINY) and (toks != r.e.cfg.eos_token_id).all()
        want = bitmap([prompt[s // G_TINY] + toks[s].tolist() for s in range(toks.shape[0])], V)
        assert tuple(r.seen.shape) == want.shape and np.array_equal(r.seen.cpu().numpy().view(np.uint32), want), call


@pytest.mark.gpu
def test_rollout_defaults_are_the_old_path():
    """generate() without the two arguments == generate(min_p=0.0, repetition_penalty=1.0): the same ids, the same captured graph, and no bitmap is allocated;
    min_p alone does not allocate one either."""
    _, r, plan, img, _ = _rollout_of(True)
    g0 = r.graph
    a = r.generate(plan, img, G_TINY, C_TINY, seed=3).cpu().numpy()
    b = r.generate(plan, img, G_TINY, C_TINY, seed=3, min_p=0.0, repetition_penalty=1.0).cpu().numpy()
    assert np.array_equal(a, b) and r.seen is None and r.graph is g0 and g0 is not None
    r.generate(plan, img, G_TINY, C_TINY, seed=3, min_p=MIN_P)
    assert r.seen is None and r.graph is not g0
    with pytest.raises(ValueError, match="min_p"):
        r.generate(plan, img, G_TINY, C_TINY, min_p=1.0)
    with pytest.raises(ValueError, match="repetition_penalty"):
        r.generate(plan, img, G_TINY, C_TINY, repetition_penalty=0.0)


@pytest.mark.gpu
def test_one_engine_step_with_both_options():
    """SCGRPOEngine.step with GRPOArgs(min_p=0.05, repetition_penalty=1.2, rollout_logps=True): a finite loss, and rollout/logp_abs_diff_* of the order of the step
    with the options off -- the sampler's log-probs are the raw row's, so they keep differing from the loss's by the engine mismatch only.  A penalty that leaked
    into them would show as |x| (1 - 1 / 1.2) on every seen token, far above a 5-fold (mean) / 10-fold (max) margin over bf16 rounding."""
    from iadr1_amd.sc_grpo import GRPOArgs, SCGRPOEngine
    reward = lambda comp: np.stack([(np.asarray(comp)[:, 0] % 5).astype(np.float32), (np.asarray(comp)[:, 1] % 3).astype(np.float32)], 1)
    m = {}
    for name, kw in (("off", {}), ("on", dict(min_p=MIN_P, repetition_penalty=1.2))):
        cfg, pol, ref, batch = _tiny()
        eng = SCGRPOEngine(cfg, pol, ref, GRPOArgs(num_generations=G_TINY, max_prompt_length=4096, max_completion_length=C_TINY, seed=5, rollout_logps=True, **kw))
        out = eng.step(batch, reward, do_optimizer_step=False, return_outputs=True)
        torch.cuda.synchronize()
        m[name] = out["metrics"]
        assert (eng._rollout.seen is not None) == (name == "on")
        print(f"[sample_ex engine step] {name}:", {k: v for k, v in m[name].items() if k.startswith("rollout/") or k == "loss"})
    assert np.isfinite(m["on"]["loss"]) and all(np.isfinite(m["on"][k]) for k in m["on"] if k.startswith("rollout/"))
    assert m["on"]["rollout/logp_abs_diff_mean"] <= 5 * m["off"]["rollout/logp_abs_diff_mean"]
    assert m["on"]["rollout/logp_abs_diff_max"] <= 10 * m["off"]["rollout/logp_abs_diff_max"]
