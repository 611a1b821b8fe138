"""iadr1_sample_guided (csrc/sample.hip): regex-guided decoding in the rollout's sampler -- a per-row automaton state, an allowed-token bitmap per state in front of
every filter, a transition table behind the pick -- and the rollout / engine layers above it.  The kernel's reference is iadr1_sample_ex itself on a copy of the
logits whose disallowed entries are -inf (bit-equal ids), the state's is trans[state, pick] on the host; the rollout's is Python's `re` on the decoded text.
Inputs are generated on the CPU, so the conditions the GPU cases rely on are asserted without one."""
import functools
import os
import re
import sys

import numpy as np
import pytest
import torch

import iadr1_amd  # noqa: F401
from iadr1_amd import guide, hip, ops

DEV = "cuda"
F32 = torch.float32
V_SMALL, V_REAL = 4099, 151936      # prime: no multiple of 32 or of the 32 chunks (csize 129), a chunk ends inside a bitmap word, the last word holds 3 ids; the real row
B, S = 4, 5
STATES = [0, 3, 3, 4]
T, MIN_P, PEN = 0.9, 0.05, 1.3
SENT = 0x5A5A5A5A
# (temperature, top_k, top_p, min_p, repetition_penalty): greedy; the top-k path; the whole vocabulary; both paths with penalty, min_p and mark_seen
PATHS = [(0.0, 1, 1.0, 0.0, 1.0), (T, 50, 0.9, 0.0, 1.0), (T, 0, 1.0, 0.0, 1.0), (T, 0, 1.0, MIN_P, PEN), (T, 50, 0.9, MIN_P, PEN)]


def words(V):
    return (V + 31) // 32


@functools.lru_cache(maxsize=None)
def inputs(V):
    """(logits [B, V] f32, allowed [S, V] bool, trans [S, V] int16, seen ids [B, 40]).  States 0, 3, 4 (the ones the rows start in) allow 30 %, 10 % and 50 % of the
    tokens but none of the top-8 of the rows that start there; states 1 and 2 allow 20 %.  trans sends an allowed token to a random state.  Never modified."""
    g = torch.Generator().manual_seed(11)
    x = (torch.randn(B, V, generator=g) * 2.5).to(F32)
    dens = torch.tensor([0.3, 0.2, 0.2, 0.1, 0.5])
    allowed = torch.rand(S, V, generator=g) < dens[:, None]
    for r, s in enumerate(STATES):
        allowed[s, x[r].topk(8).indices] = False
    nxt = torch.randint(0, S, (S, V), generator=g).to(torch.int16)
    trans = torch.where(allowed, nxt, torch.full_like(nxt, -1))
    seen = torch.cat([torch.randint(0, V, (B, 37), generator=g), torch.stack([(x[r].masked_fill(~allowed[STATES[r]], -np.inf)).topk(3).indices for r in range(B)])], 1)
    return x.numpy(), allowed.numpy(), trans.numpy(), seen.numpy()


def bitmap(mask, ld):
    """[rows, V] bool -> [rows, ld] uint32, bit id & 31 of word id >> 5."""
    rows, V = mask.shape
    bm = np.zeros((rows, ld * 32), dtype=bool)
    bm[:, :V] = mask
    return np.packbits(bm, axis=1, bitorder="little").view("<u4").astype(np.uint32)


def framed(a):
    """A [rows, ld] (or [n]) array inside a larger allocation, 8 sentinel elements in front and behind: (whole flat device buffer, the view the kernels get)."""
    a = np.ascontiguousarray(a)
    sent = np.array([SENT], dtype=np.uint32).view(a.dtype if a.dtype.itemsize == 4 else np.int16)[0]
    buf = np.full(16 + a.size, sent, dtype=a.dtype)
    buf[8: 8 + a.size] = a.reshape(-1)
    whole = torch.from_numpy(buf.view({4: np.int32, 2: np.int16}[a.dtype.itemsize]).copy()).to(DEV)
    return whole, whole[8: 8 + a.size].view(a.shape)


def unframed(whole, like):
    a = whole.cpu().numpy().view(like.dtype)
    sent = np.array([SENT], dtype=np.uint32).view(like.dtype if like.dtype.itemsize == 4 else np.int16)[0]
    assert (a[:8] == sent).all() and (a[-8:] == sent).all(), "a write outside the buffer"
    return a[8:-8].reshape(like.shape)


class Tables:
    """allow / trans / state on the device, each in its sentinel frame and with a leading dimension larger than needed."""

    def __init__(self, allowed, trans, states):
        Sx, V = allowed.shape
        self.allow_h = bitmap(allowed, words(V) + 3)
        self.trans_h = np.full((Sx, V + 5), -1, dtype=np.int16)
        self.trans_h[:, :V] = trans
        self.state_h = np.asarray(states, dtype=np.int32)
        self.wa, self.allow = framed(self.allow_h)
        self.wt, self.trans = framed(self.trans_h)
        self.ws, self.state = framed(self.state_h)
        self.trans = self.trans[:, :]          # ld_trans = V + 5 through the row stride

    def kw(self):
        return dict(state=self.state, allow=self.allow, trans=self.trans)

    def check_frames(self):
        assert np.array_equal(unframed(self.wa, self.allow_h), self.allow_h), "allow was written"
        assert np.array_equal(unframed(self.wt, self.trans_h), self.trans_h), "trans was written"
        return unframed(self.ws, self.state_h).copy()


def seen_dev(ids, V):
    m = np.zeros((len(ids), V), dtype=bool)
    for r, row in enumerate(ids):
        m[r, row] = True
    return torch.from_numpy(bitmap(m, words(V)).view(np.int32).copy()).to(DEV)


def ref_logp(lg, ids):
    return torch.log_softmax(lg.double(), -1).gather(1, ids.view(-1, 1)).squeeze(1)


def close(got, ref, rtol, atol, what=""):
    got, ref = got.double().cpu(), ref.double().cpu()
    err = (got - ref).abs()
    tol = atol + rtol * ref.abs()
    assert not bool((err > tol).any()), f"{what}: {int((err > tol).sum())}/{ref.numel()} out of tol, max|err| {err.max().item():.4g}"


def call(lg, path, tb, seed=77, step=0, seen=None, **kw):
    T_, k, p, mp, pen = path
    return ops.sample_guided(lg, T_, k, p, seed=seed, step=step, min_p=mp, repetition_penalty=pen, seen=seen if pen != 1.0 else None, mark_seen=pen != 1.0,
                             **(tb.kw() if tb is not None else {}), **kw)


# ---- without a GPU -------------------------------------------------------------------------------------------------------------------------------------------

def test_abi_has_the_entry_point():
    L = hip.lib()
    assert hip.version() >= 116
    for name in ("iadr1_sample_guided", "iadr1_sample_guided_workspace_bytes"):
        assert name in hip.PROTOS and hasattr(L, name)
    assert L.iadr1_sample_guided_workspace_bytes(64) >= L.iadr1_sample_ex_workspace_bytes(64)
    names = [a for _, a in hip.PROTOS["iadr1_sample_guided"][1]]
    assert names[:len(hip.PROTOS["iadr1_sample_ex"][1]) - 1] == [a for _, a in hip.PROTOS["iadr1_sample_ex"][1]][:-1], "everything iadr1_sample_ex takes, in its order"
    assert names[-7:] == ["state", "allow", "ld_allow", "trans", "ld_trans", "S", "stream"]


def _guided(L, *, B_=1, V=64, T_=0.9, k=50, p=0.9, min_p=0.0, pen=1.0, seen=None, ld_seen=0, mark=0, state=None, allow=None, ld_allow=0, trans=None, ld_trans=0, S_=0):
    rc = L.iadr1_sample_guided(None, 0, None, None, 0, 0, None, B_, V, T_, k, p, min_p, pen, seen, ld_seen, mark, -1, 0, 0, None, None, state, allow, ld_allow, trans, ld_trans, S_, None)
    return rc, L.iadr1_last_error()


def test_host_refusals_each_have_their_own_message_without_a_gpu():
    """Every refusal is detected before any launch (no device buffer exists: the non-NULL pointers are refused before anything could read them): rc < 0 and a
    message of its own, prefixed sample_guided:."""
    L = hip.lib()
    some = 0x1000
    ok = dict(state=some, allow=some, ld_allow=2, trans=some, ld_trans=64, S_=3)
    msgs = []

    def refused(word, **kw):
        rc, m = _guided(L, **kw)
        assert rc < 0 and m.startswith(b"sample_guided:") and word in m, (kw, m)
        return m

    for kw in (dict(ok, state=None), dict(ok, trans=None), dict(ok, state=None, trans=None)):
        m = refused(b"allow needs state", **kw)
    msgs.append(m)
    for kw in (dict(state=some), dict(trans=some, ld_trans=64), dict(state=some, trans=some, S_=3)):
        m = refused(b"must be NULL when allow is NULL", **kw)
    msgs.append(m)
    for s_ in (0, -1, 32768, 1 << 20):
        m = refused(b"outside 1..32767", **dict(ok, S_=s_))
    msgs.append(m)
    msgs.append(refused(b"ld_allow=1 is less than ceil(V / 32) = 2", **dict(ok, ld_allow=1)))
    msgs.append(refused(b"ld_allow", V=65, **dict(ok, ld_trans=65)))
    msgs.append(refused(b"ld_trans=63 is less than V = 64", **dict(ok, ld_trans=63)))
    # everything iadr1_sample_ex refuses, with and without a guide
    for extra in (ok, {}):
        msgs.append(refused(b"min_p must be in", min_p=1.0, **extra))
        msgs.append(refused(b"repetition_penalty must be finite", pen=float("inf"), **extra))
        msgs.append(refused(b"seen bitmap", pen=1.3, **extra))
        msgs.append(refused(b"seen bitmap", mark=1, seen=some, ld_seen=1, **extra))
        msgs.append(refused(b"nucleus", k=0, p=0.9, **extra))
        msgs.append(refused(b"top_p must be in", p=0.0, **extra))
        msgs.append(refused(b"empty problem", B_=0, **extra))
        msgs.append(refused(b"empty problem or missing workspace", **extra))       # (all checks passed but the workspace: nothing was launched)
    # (V and top_k beyond the built maxima are checked behind the workspace, as in iadr1_sample_ex: they cannot be reached without a buffer)
    assert len(set(msgs)) == 6 + 7      # the five guide refusals (ld_allow with two pairs of numbers) and seven of iadr1_sample_ex's: all different texts


@pytest.mark.parametrize("V", [V_SMALL, V_REAL])
def test_conditions_of_the_gpu_cases_hold_on_these_inputs(V):
    """Conditions, not measurements: (a) every state keeps at least 2 allowed tokens with a finite logit in every row (whichever state the chain reaches);
    (b) the unguided pick -- the argmax for greedy, and every one of the top-8 that carry most of the top-k / whole-vocabulary mass -- is a DISALLOWED token in
    every row (the issue asks for half), so a mask that is silently ignored cannot pass; (c) the guided greedy pick differs from the unguided one in every row."""
    x, allowed, trans, seen = inputs(V)
    assert allowed.shape == (S, V) and ((trans >= 0) == allowed).all() and trans.max() < S
    for s in range(S):
        for r in range(B):
            keep = allowed[s] & np.isfinite(x[r])
            assert keep.sum() >= 2, (s, r)
    off = 0
    for r, s in enumerate(STATES):
        top = np.argsort(-x[r])[:8]
        assert not allowed[s, top].any()
        off += not allowed[s, x[r].argmax()]
        assert np.where(allowed[s], x[r], -np.inf).argmax() != x[r].argmax()
    assert off >= B // 2 and off == B
    if V == V_SMALL:
        assert V % 32 == 3, "the last bitmap word holds 3 ids"
        csize = (V + 31) // 32
        assert any((c * csize) % 32 for c in range(1, 32)), "a chunk ends inside a bitmap word"


# ---- the kernels -----------------------------------------------------------------------------------------------------------------------------------------------

def masked_copy(x, allowed, states):
    xm = x.copy()
    for r, s in enumerate(states):
        xm[r, ~allowed[s]] = -np.inf
    return xm


@pytest.mark.gpu
@pytest.mark.parametrize("V,steps", [(V_SMALL, 16), (V_REAL, 4)])
def test_guided_ids_are_sample_ex_on_the_masked_row(V, steps):
    """(1) Chained steps, five paths: ids bit-equal to iadr1_sample_ex on a copy of the logits with the disallowed entries of every row's CURRENT state at -inf (same
    seed, same step, its own seen bitmap); after every step state == trans[state_before, pick] exactly, and allow, trans and all sentinels are as they were."""
    x, allowed, trans, seen_ids = inputs(V)
    lg = torch.from_numpy(x).to(DEV)
    for path in PATHS:
        tb = Tables(allowed, trans, STATES)
        seen_a, seen_b = seen_dev(seen_ids, V), seen_dev(seen_ids, V)
        T_, k, p, mp, pen = path
        visited = set()
        for step in range(steps):
            before = tb.check_frames()
            visited |= set(before.tolist())
            ref_lg = torch.from_numpy(masked_copy(x, allowed, before)).to(DEV)
            want = ops.sample_ex(ref_lg, T_, k, p, seed=77, step=step, min_p=mp, repetition_penalty=pen, seen=seen_b if pen != 1.0 else None, mark_seen=pen != 1.0, want_logp=False)[0]
            got = call(lg, path, tb, step=step, seen=seen_a, want_logp=False)[0]
            assert torch.equal(got, want), (V, path, step, got.tolist(), want.tolist(), before.tolist())
            picks = got.cpu().numpy()
            assert allowed[before, picks].all()
            after = tb.check_frames()
            assert np.array_equal(after, trans[before, picks].astype(np.int32)), (V, path, step)
            assert torch.equal(seen_a, seen_b)
        assert len(visited) >= 3, "the chain stayed where it started"


@pytest.mark.gpu
def test_logp_stays_the_raw_row_log_softmax():
    """(2) logp_out is the float64 log-softmax of the RAW row at the pick -- no mask, no penalty, no filter -- at test_sample_ex's bound for the same quantity
    (1e-5, 1e-5).  The masked row's log-softmax at the pick is several nats away (the mask removes the row's top-8 and 50 - 90 % of the mass), asserted too."""
    x, allowed, trans, seen_ids = inputs(V_SMALL)
    lg = torch.from_numpy(x).to(DEV)
    for path in PATHS:
        tb = Tables(allowed, trans, STATES)
        got, lp = call(lg, path, tb, seed=99, seen=seen_dev(seen_ids, V_SMALL))
        assert lp.shape == (B, 1)
        close(lp[:, 0], ref_logp(lg, got), 1e-5, 1e-5, f"logp {path}")
        masked = ref_logp(torch.from_numpy(masked_copy(x, allowed, STATES)).to(DEV), got)
        assert bool(((lp[:, 0].double().cpu() - masked.cpu()).abs() > 0.5).all())
    buf = torch.full((B, 6), 7.0, device=DEV)
    sp = torch.tensor([4], dtype=torch.int32, device=DEV)
    tb = Tables(allowed, trans, STATES)
    got, _ = call(lg, PATHS[3], tb, seed=3, seen=seen_dev(seen_ids, V_SMALL), step_ptr=sp, logp_out=buf)
    close(buf[:, 4], ref_logp(lg, got), 1e-5, 1e-5, "column from step_ptr")
    assert bool((buf[:, [0, 1, 2, 3, 5]] == 7.0).all())


@pytest.mark.gpu
def test_single_allowed_token_and_last_partial_word():
    """(3) State 1 allows ONE token, whose logit is the row's minimum while the row's argmax is disallowed: every path returns exactly that token.  (4) State 2
    allows only the three ids of the last, partial bitmap word of the last chunk (4096..4098): every path returns one of them, greedy the largest of the three,
    and the ids equal the masked-row reference.  Both advance along trans."""
    V = V_SMALL
    x, allowed, trans, seen_ids = inputs(V)
    x, allowed, trans = x.copy(), allowed.copy(), trans.copy()
    one = 1234
    x[:, one] = x.min(1) - 1.0
    allowed[1] = False
    allowed[1, one] = True
    allowed[2] = False
    allowed[2, 4096:] = True
    assert words(V) * 32 - V == 29 and allowed[2].sum() == 3
    trans[1], trans[2] = -1, -1
    trans[1, one], trans[2, 4096:] = 4, [0, 3, 4]
    states = [1, 2, 1, 2]
    lg = torch.from_numpy(x).to(DEV)
    ref_lg = torch.from_numpy(masked_copy(x, allowed, states)).to(DEV)
    for path in PATHS:
        T_, k, p, mp, pen = path
        for step in range(4):
            tb = Tables(allowed, trans, states)
            got = call(lg, path, tb, step=step, seen=seen_dev(seen_ids, V), want_logp=False)[0].cpu().numpy()
            assert got[0] == one and got[2] == one and 4096 <= got[1] < V and 4096 <= got[3] < V, (path, step, got)
            want = ops.sample_ex(ref_lg, T_, k, p, seed=77, step=step, min_p=mp, repetition_penalty=pen, seen=seen_dev(seen_ids, V) if pen != 1.0 else None, want_logp=False)[0]
            assert np.array_equal(got, want.cpu().numpy())
            if T_ == 0.0:
                assert got[1] == 4096 + x[1, 4096:].argmax() and got[3] == 4096 + x[3, 4096:].argmax()
            assert np.array_equal(tb.check_frames(), trans[states, got].astype(np.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("V", [V_SMALL, V_REAL])
def test_no_guide_is_bit_equal_to_sample_ex(V):
    """(5) allow = state = trans = NULL: ids and logp_out bit-equal to iadr1_sample_ex, seen marked the same way."""
    x, _, _, seen_ids = inputs(V)
    lg = torch.from_numpy(x).to(DEV)
    for path in PATHS:
        T_, k, p, mp, pen = path
        for step in range(3):
            seen_a, seen_b = seen_dev(seen_ids, V), seen_dev(seen_ids, V)
            a, la = ops.sample_ex(lg, T_, k, p, seed=5, step=step, min_p=mp, repetition_penalty=pen, seen=seen_a if pen != 1.0 else None, mark_seen=pen != 1.0, logp_out=torch.zeros(B, 4, device=DEV))
            b, lb = call(lg, path, None, seed=5, step=step, seen=seen_b, logp_out=torch.zeros(B, 4, device=DEV))
            assert torch.equal(a, b) and torch.equal(la, lb) and torch.equal(seen_a, seen_b), (V, path, step)


@pytest.mark.gpu
def test_all_allowed_logits_minus_inf_keeps_the_state():
    """(6) Rows 1 and 2 are in a state whose allowed tokens (three ids far from the low ids the sampler's fallbacks return) all hold -inf: the returned id is in
    [0, V) and disallowed, so the state stays where it was; the other rows advance as usual; nothing outside the buffers is written."""
    V = V_SMALL
    x, allowed, trans, seen_ids = inputs(V)
    x, allowed, trans = x.copy(), allowed.copy(), trans.copy()
    dead = [1000, 2000, 3000]
    allowed[3] = False
    allowed[3, dead] = True
    trans[3] = -1
    trans[3, dead] = 1
    x[1, dead] = x[2, dead] = -np.inf
    lg = torch.from_numpy(x).to(DEV)
    for path in PATHS:
        tb = Tables(allowed, trans, STATES)
        got = call(lg, path, tb, seen=seen_dev(seen_ids, V), want_logp=False)[0].cpu().numpy()
        assert ((got >= 0) & (got < V)).all(), (path, got)
        after = tb.check_frames()
        assert after[1] == 3 and after[2] == 3, (path, got, after)
        assert after[0] == trans[0, got[0]] and after[3] == trans[4, got[3]] and allowed[0, got[0]] and allowed[4, got[3]]


# ---- rollout and engine (the TINY fixture model; the character-level tokenizer of tests/fixture_util.py) -------------------------------------------------------

PATTERN = r"<loc>(top|bottom) (left|right)</loc><n>[0-9]{1,3}</n><ans>(yes|no)</ans>"
LONGEST, SHORTEST = len("<loc>bottom right</loc><n>123</n><ans>yes</ans>"), len("<loc>top left</loc><n>1</n><ans>no</ans>")
G_TINY, C_TINY = 4, LONGEST + 2


def _fx():
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import fixture_util as fx
    return fx


@functools.lru_cache(maxsize=None)
def tiny_guide():
    """(guide, byte string per token id): the pattern over the fixture's character tokenizer -- printable ASCII and \\n, the Qwen2-VL specials unemittable -- with
    the TINY model's EOS id and vocabulary size (640: ids beyond the tokenizer's 103 are padding)."""
    fx = _fx()
    tb = guide.token_bytes(fx.local_qwen2vl_processor().tokenizer, fx.TINY["text"]["vocab_size"])
    return guide.TokenGuide.build(guide.compile_regex(PATTERN), tb, fx.TINY["eos_token_id"], fx.TINY["text"]["vocab_size"]), tb


def _tiny():
    fx = _fx()
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


def _rollout_of(use_graph=True, **kw):
    """(engine, its Rollout, plan, image embeddings): one default rollout through the engine builds the pool (and, with use_graph, captures the default step)."""
    from iadr1_amd.sc_grpo import GRPOArgs, SCGRPOEngine
    cfg, pol, ref, batch = _tiny()
    eng = SCGRPOEngine(cfg, pol, ref, GRPOArgs(num_generations=G_TINY, max_prompt_length=4096, max_completion_length=C_TINY, seed=5, use_hip_graph=use_graph, **kw))
    eng.rollout(batch)
    vis = eng.vision_policy(batch, save=False)
    gpr, off = eng._per_row_images(batch, vis["grids"], vis["rows"])
    plan = eng.pol.text_plan(np.asarray(batch["input_ids"]), np.asarray(batch["attention_mask"]), gpr, off)
    return eng, eng._rollout, plan, vis["img"]


def check_rows(toks, cfg, expect_eos):
    """Every row that emitted EOS decodes (specials skipped) to a full match and holds nothing but pad behind the EOS; every other row is a prefix from which the
    DFA can still accept.  Returns the number of rows that ended."""
    g, tb = tiny_guide()
    rx = re.compile(PATTERN)
    ended = 0
    for row in np.asarray(toks).tolist():
        if cfg.eos_token_id in row:
            n = row.index(cfg.eos_token_id)
            text = b"".join(tb[t] or b"" for t in row[:n]).decode()
            assert rx.fullmatch(text), text
            assert all(t == cfg.pad_token_id for t in row[n + 1:]), row
            ended += 1
        else:
            assert all(tb[t] is not None for t in row), row
            assert g.dfa.live(b"".join(tb[t] for t in row)), row
    assert expect_eos is None or (ended == len(toks)) == expect_eos
    return ended


def test_the_rollout_pattern_over_the_fixture_tokenizer():
    """Without a GPU: the guide of the rollout cases exists, knows the longest and the shortest match, and an EOS is allowed only behind a match."""
    g, tb = tiny_guide()
    fx = _fx()
    assert g.V == 640 and g.eos_id == fx.TINY["eos_token_id"] and tb[fx.TINY["eos_token_id"]] is None and tb[fx.TINY["pad_token_id"]] is None
    enc = lambda s: [tb.index(bytes([c])) for c in s.encode()]
    for text in ("<loc>bottom right</loc><n>123</n><ans>yes</ans>", "<loc>top left</loc><n>1</n><ans>no</ans>"):
        s = g.walk(enc(text))
        assert s >= 0 and g.accepting[s] and g.walk(enc(text) + [g.eos_id]) == s and g.walk(enc(text[:-1]) + [g.eos_id]) == -1
        assert (g.trans[s] >= 0).sum() == 1, "behind a match only EOS is allowed: a row given LONGEST + 1 tokens always ends"
    assert g.walk(enc("<loc>left")) == -1 and g.walk(enc("<loc>top left</loc><n>1234")) == -1


@pytest.mark.gpu
def test_guided_rollout_matches_and_live_prefixes():
    """(7) Sampled at T = 0.9 / top-k 50 and over the whole vocabulary with min_p and a penalty: with max_new = LONGEST + 2 every row ends in an EOS behind a full
    match of the pattern; with max_new below the shortest match every row is a live prefix without an EOS.  Random weights never produce a match unguided."""
    eng, r, plan, img = _rollout_of(True)
    g, _ = tiny_guide()
    cfg = r.e.cfg
    plain = r.generate(plan, img, G_TINY, C_TINY, seed=9).cpu().numpy()
    with pytest.raises(AssertionError):
        check_rows(plain, cfg, None)
    for kw in (dict(), dict(top_k=0, top_p=1.0, min_p=MIN_P, repetition_penalty=1.2), dict(temperature=0.0, top_k=1, top_p=1.0)):
        toks = r.generate(plan, img, G_TINY, C_TINY, seed=9, guide=g, **kw).cpu().numpy()
        assert toks.shape == (2 * G_TINY, C_TINY)
        assert check_rows(toks, cfg, True) == 2 * G_TINY
        short = r.generate(plan, img, G_TINY, SHORTEST - 5, seed=9, guide=g, **kw).cpu().numpy()
        assert check_rows(short, cfg, False) == 0
    with pytest.raises(ValueError, match="suppress_eos"):
        r.generate(plan, img, G_TINY, C_TINY, guide=g, suppress_eos=True)


@pytest.mark.gpu
def test_guided_rollout_graph_and_eager_give_the_same_ids():
    """(8) Identical ids from the captured graph and from eager launches (the capture's two extra steps leave no mark on the automaton state); a second rollout on
    the same object with another seed is valid too and differs -- a state left over from the first one would not be a start state."""
    g, _ = tiny_guide()
    got = {}
    for use_graph in (True, False):
        _, r, plan, img = _rollout_of(use_graph)
        a = r.generate(plan, img, G_TINY, C_TINY, seed=9, guide=g).cpu().numpy()
        assert (r.graph is not None) == use_graph and r.g_state is not None
        graph = r.graph
        b = r.generate(plan, img, G_TINY, C_TINY, seed=10, guide=g).cpu().numpy()
        assert r.graph is graph, "the same guide object: no new upload, no new capture"
        check_rows(a, r.e.cfg, True)
        check_rows(b, r.e.cfg, True)
        assert not np.array_equal(a, b)
        assert np.array_equal(a, r.generate(plan, img, G_TINY, C_TINY, seed=9, guide=g).cpu().numpy())
        got[use_graph] = (a, b)
    assert np.array_equal(got[True][0], got[False][0]) and np.array_equal(got[True][1], got[False][1])


@pytest.mark.gpu
def test_guide_off_again_is_the_old_path(monkeypatch):
    """(9) A guided rollout, then one without: ids bit-equal to the unguided rollout before it and to a fresh Rollout's.  With the guided entry point made to
    raise, default rollouts (graph and eager) still run: they do not go through it."""
    g, _ = tiny_guide()
    _, r, plan, img = _rollout_of(True)
    before = r.generate(plan, img, G_TINY, C_TINY, seed=3).cpu().numpy()
    r.generate(plan, img, G_TINY, C_TINY, seed=3, guide=g)
    after = r.generate(plan, img, G_TINY, C_TINY, seed=3).cpu().numpy()
    assert np.array_equal(before, after) and r.sampling["guided"] is False
    monkeypatch.setattr(ops, "sample_guided", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the default rollout took the guided path")))
    for use_graph in (True, False):
        _, r2, plan2, img2 = _rollout_of(use_graph)
        assert r2.guide is None and r2.g_state is None
        assert np.array_equal(r2.generate(plan2, img2, G_TINY, C_TINY, seed=3).cpu().numpy(), before)


@pytest.mark.gpu
def test_one_engine_step_with_the_guide():
    """(10) SCGRPOEngine.step with GRPOArgs(guide=..., rollout_logps=True): a finite loss, completions that match, and rollout/logp_abs_diff_* of the order of the
    step without the guide -- the sampler's log-probs are the raw row's.  A mask that leaked into them would renormalise over the one to ten allowed characters:
    several nats on every token, far above a 5-fold (mean) / 10-fold (max) margin over bf16 rounding."""
    from iadr1_amd.sc_grpo import GRPOArgs, SCGRPOEngine
    g, _ = tiny_guide()
    reward = lambda comp: np.stack([(np.asarray(comp)[:, 0] % 5).astype(np.float32), (np.asarray(comp)[:, 1] % 3).astype(np.float32)], 1)
    m = {}
    for name, kw in (("off", {}), ("on", dict(guide=g))):
        cfg, pol, ref, batch = _tiny()
        eng = SCGRPOEngine(cfg, pol, ref, GRPOArgs(num_generations=G_TINY, max_prompt_length=4096, max_completion_length=C_TINY, seed=5, rollout_logps=True, **kw))
        out = eng.step(batch, reward, do_optimizer_step=False, return_outputs=True)
        torch.cuda.synchronize()
        m[name] = out["metrics"]
        assert (eng._rollout.guide is not None) == (name == "on")
        if name == "on":
            check_rows(eng._rollout.tokens_host(), cfg, True)
        print(f"[sample_guided engine step] {name}:", {k: v for k, v in m[name].items() if k.startswith("rollout/") or k == "loss"})
    assert np.isfinite(m["on"]["loss"]) and all(np.isfinite(m["on"][k]) for k in m["on"] if k.startswith("rollout/"))
    assert m["on"]["rollout/logp_abs_diff_mean"] <= 5 * m["off"]["rollout/logp_abs_diff_mean"]
    assert m["on"]["rollout/logp_abs_diff_max"] <= 10 * m["off"]["rollout/logp_abs_diff_max"]
