"""iadr1_sample_ent (csrc/sample.hip, the EN flag of stage1 / stage2): the entropy of the distribution every token is sampled from -- softmax of the RAW fp32 row at
temperature 1, nothing suppressed, masked, penalised or filtered -- beside everything iadr1_sample_guided returns.  The reference of the entropy is float64 numpy,
written here; the reference of ids, log-probs, seen bitmap and automaton state is ops.sample_guided on the same arguments (bit-equal).  Inputs are generated on the
CPU, so what the GPU cases rely on (a kernel that took the entropy of another distribution cannot pass) is asserted without one."""
import functools

import numpy as np
import pytest
import torch

import iadr1_amd  # noqa: F401
from iadr1_amd import hip, ops

DEV = "cuda"
F32 = torch.float32
B = 8
SIZES = [640, 20011, 151936]        # one id per thread; prime, slices straddle; the real row
RANDN_ROWS = (0, 3, 4, 5, 7)        # the rows that are (scaled / partly masked) gaussians: 1 is a spike, 2 a constant, 6 nearly flat
RTOL = ATOL = 1e-5                  # what the project holds iadr1_logprob_rows and logp_out to
T, MIN_P, PEN = 0.9, 0.05, 1.3
SENT = -7.25                        # sentinel of the framed entropy buffer: no entropy is negative
# (name, temperature, top_k, top_p, min_p, repetition_penalty, guided)
CASES = [("topk_topp", T, 50, 0.9, 0.0, 1.0, False), ("greedy", 0.0, 1, 1.0, 0.0, 1.0, False), ("whole_vocab", T, 0, 1.0, 0.0, 1.0, False),
         ("penalty_min_p", T, 50, 0.9, MIN_P, PEN, False), ("whole_vocab_penalty_min_p", T, 0, 1.0, MIN_P, PEN, False), ("guided", T, 50, 0.9, 0.0, 1.0, True),
         ("guided_whole_vocab", T, 0, 1.0, 0.0, 1.0, True)]


@functools.lru_cache(maxsize=None)
def inputs(V):
    """logits [B, V] float32 (numpy, never modified): gaussians * 2.5, then row 1 one logit of 50 (H ~ 0), row 2 constant (H = ln V), row 3 its first two whole
    chunks at -inf, row 4 every third id at -inf, row 5 x 4 (sharp), row 6 x 0.05 (flat)."""
    x = (torch.randn(B, V, generator=torch.Generator().manual_seed(1)) * 2.5).to(F32).numpy().copy()
    x[1, V // 3] = 50.0
    x[2, :] = 0.75
    x[3, : 2 * ((V + 31) // 32)] = -np.inf
    x[4, ::3] = -np.inf
    x[5] *= 4.0
    x[6] *= 0.05
    return x


def entropy64(x):
    """H = -sum p ln p of softmax(row) in float64; p == 0 (a logit of -inf) contributes 0."""
    x = np.asarray(x, dtype=np.float64)
    z = x - x.max(-1, keepdims=True)
    e = np.exp(z)
    s = e.sum(-1, keepdims=True)
    with np.errstate(invalid="ignore"):
        t = np.where(e > 0, (e / s) * (z - np.log(s)), 0.0)
    return -t.sum(-1)


def words(V):
    return (V + 31) // 32


def bitmap(mask, ld):
    """[rows, V] bool -> [rows, ld] int32, bit id & 31 of word id >> 5."""
    rows, V = mask.shape
    bm = np.zeros((rows, ld * 32), dtype=bool)
    bm[:, :V] = mask
    return np.packbits(bm, axis=1, bitorder="little").view("<u4").view(np.int32).copy()


@functools.lru_cache(maxsize=None)
def tables(V):
    """A 2-state guide (allowed [2, V] bool, trans [2, V] int16, start states [B]) and the seen ids of the penalty [B, 40]; no row's top-8 is allowed in its state."""
    g = torch.Generator().manual_seed(23)
    x = inputs(V)
    allowed = (torch.rand(2, V, generator=g) < 0.4).numpy()
    states = np.arange(B, dtype=np.int32) % 2
    for r in range(B):
        allowed[states[r], np.argsort(-x[r])[:8]] = False
    nxt = torch.randint(0, 2, (2, V), generator=g).to(torch.int16).numpy()
    trans = np.where(allowed, nxt, np.int16(-1)).astype(np.int16)
    seen = np.concatenate([torch.randint(0, V, (B, 37), generator=g).numpy(), np.argsort(-x, 1)[:, :3]], 1)
    return allowed, trans, states, seen


def device_args(V, case):
    """Fresh device-side keyword arguments of one case (the sampler writes seen and state)."""
    _, T_, k, p, mp, pen, guided = case
    allowed, trans, states, seen_ids = tables(V)
    kw = dict(min_p=mp, repetition_penalty=pen)
    if pen != 1.0:
        m = np.zeros((B, V), dtype=bool)
        for r in range(B):
            m[r, seen_ids[r]] = True
        kw.update(seen=torch.from_numpy(bitmap(m, words(V))).to(DEV), mark_seen=True)
    if guided:
        kw.update(state=torch.from_numpy(states.copy()).to(DEV), allow=torch.from_numpy(bitmap(allowed, words(V))).to(DEV), trans=torch.from_numpy(trans.copy()).to(DEV))
    return (T_, k, p), kw


def close(got, ref, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    err = np.abs(got - ref)
    tol = ATOL + RTOL * np.abs(ref)
    print(f"[sample_ent] {what}: max |H - H64| {err.max():.3e}, max err / tol {(err / tol).max():.3f}")
    assert (err <= tol).all(), f"{what}: rows {np.flatnonzero(err > tol).tolist()} out of tolerance, max |err| {err.max():.4g}, H64 {ref.tolist()}, got {got.tolist()}"


# ---- without a GPU -------------------------------------------------------------------------------------------------------------------------------------------

def test_abi_has_the_entry_points():
    L = hip.lib()
    assert hip.version() >= 117
    for name in ("iadr1_sample_ent", "iadr1_sample_ent_workspace_bytes", "iadr1_grpo_loss_sel"):
        assert name in hip.PROTOS and hasattr(L, name)
    assert L.iadr1_sample_ent_workspace_bytes(64) == L.iadr1_sample_guided_workspace_bytes(64) + 64 * 32 * 4 > L.iadr1_sample_guided_workspace_bytes(64)
    names = [a for _, a in hip.PROTOS["iadr1_sample_ent"][1]]
    assert names[:-4] == [a for _, a in hip.PROTOS["iadr1_sample_guided"][1]][:-1], "everything iadr1_sample_guided takes, in its order"
    assert names[-4:] == ["ent_out", "ld_ent", "ent_cols", "stream"]
    assert [a for _, a in hip.PROTOS["iadr1_grpo_loss_sel"][1]][:-2] == [a for _, a in hip.PROTOS["iadr1_grpo_loss_ex"][1]][:-1]
    assert [a for _, a in hip.PROTOS["iadr1_grpo_loss_sel"][1]][-2:] == ["sel", "stream"]


def _ent(L, *, B_=1, V=64, T_=0.9, k=50, p=0.9, min_p=0.0, pen=1.0, seen=None, ld_seen=0, mark=0, state=None, allow=None, ld_allow=0, trans=None, ld_trans=0, S_=0, ent=None,
         ld_ent=0, cols=0):
    rc = L.iadr1_sample_ent(None, 0, None, None, 0, 0, None, B_, V, T_, k, p, min_p, pen, seen, ld_seen, mark, -1, 0, 0, None, None, state, allow, ld_allow, trans, ld_trans, S_,
                            ent, ld_ent, cols, None)
    return rc, L.iadr1_last_error()


def test_host_refusals_each_have_their_own_message_without_a_gpu():
    """Every refusal is detected before any launch (no device buffer exists: the non-NULL pointers are refused before anything could read them): rc < 0 and a
    message of its own, prefixed sample_ent:."""
    L = hip.lib()
    some = 0x1000
    guide = dict(state=some, allow=some, ld_allow=2, trans=some, ld_trans=64, S_=3)
    ent = dict(ent=some, ld_ent=4, cols=4)
    msgs = []

    def refused(word, **kw):
        rc, m = _ent(L, **kw)
        assert rc < 0 and m.startswith(b"sample_ent:") and word in m, (kw, m)
        return m

    for c in (0, -3):
        m = refused(b"ent_out needs ent_cols > 0", **dict(ent, cols=c))
    msgs.append(m)
    msgs.append(refused(b"ld_ent=3 is less than ent_cols = 4", **dict(ent, ld_ent=3)))
    msgs.append(refused(b"ld_ent=0 is less than ent_cols = 1", **dict(ent, ld_ent=0, cols=1), **guide))
    # everything iadr1_sample_guided refuses, with and without the entropy output
    for extra in (ent, {}):
        msgs.append(refused(b"allow needs state", **dict(guide, state=None), **extra))
        msgs.append(refused(b"must be NULL when allow is NULL", state=some, **extra))
        msgs.append(refused(b"outside 1..32767", **dict(guide, S_=0), **extra))
        msgs.append(refused(b"ld_allow=1 is less than ceil(V / 32) = 2", **dict(guide, ld_allow=1), **extra))
        msgs.append(refused(b"ld_trans=63 is less than V = 64", **dict(guide, ld_trans=63), **extra))
        msgs.append(refused(b"min_p must be in", min_p=1.0, **extra))
        msgs.append(refused(b"repetition_penalty must be finite", pen=float("inf"), **extra))
        msgs.append(refused(b"seen bitmap", pen=1.3, **extra))
        msgs.append(refused(b"nucleus", k=0, p=0.9, **extra))          # the whole-vocabulary nucleus stays refused
        msgs.append(refused(b"top_p must be in", p=0.0, **extra))
        msgs.append(refused(b"empty problem or missing workspace (iadr1_sample_ent_workspace_bytes)", **extra))   # (all checks passed but the workspace: nothing was launched)
    assert len(set(msgs)) == 3 + 11


@pytest.mark.parametrize("V", SIZES)
def test_fault_model_of_the_inputs(V):
    """Conditions of the GPU cases, not measurements: on the gaussian-type rows the float64 entropy of the raw row differs from the entropy at T = 0.9 and from
    the entropy with the row argmax suppressed by more than 100 x the tolerance, so a kernel that takes the entropy of the filter's distribution cannot pass; the
    special rows are what their names say; row 3 starts with two whole all--inf chunks."""
    x = inputs(V)
    H = entropy64(x)
    tol = ATOL + RTOL * np.abs(H)
    Ht = entropy64(x.astype(np.float64) / T)
    xs = x.copy()
    xs[np.arange(B), x.argmax(1)] = -np.inf
    Hs = entropy64(xs)
    rt, rs = np.abs(Ht - H) / tol, np.abs(Hs - H) / tol
    print(f"[sample_ent] V={V}: H64 {np.round(H, 4).tolist()}; |H(T=0.9) - H| / tol {np.round(rt).tolist()}; |H(argmax suppressed) - H| / tol {np.round(rs).tolist()}")
    for r in RANDN_ROWS:
        assert rt[r] > 100 and rs[r] > 100, (r, rt[r], rs[r])
    assert H[1] < 1e-3 and abs(H[2] - np.log(V)) < 1e-9 and H[6] > np.log(V) - 0.05 and (H >= 0).all() and (H <= np.log(V) + 1e-12).all()
    csize = (V + 31) // 32
    assert np.isneginf(x[3, : 2 * csize]).all() and np.isfinite(x[3, 2 * csize:]).all() and np.isneginf(x[4, ::3]).all()
    # a float32 restatement of the kernel's formula (per-chunk partials, then the merge) stays far inside the tolerance: the bound is derivable, not fitted
    x32 = np.pad(x, ((0, 0), (0, 32 * csize - V)), constant_values=-np.inf).reshape(B, 32, csize)
    with np.errstate(invalid="ignore", over="ignore"):
        m1 = x32.max(-1)
        d = (x32 - m1[..., None]).astype(np.float32)
        ok = np.isfinite(d)
        e = np.where(ok, np.exp(d, dtype=np.float32), np.float32(0))
        s1, u1 = e.sum(-1, dtype=np.float32), np.where(ok, e * d, np.float32(0)).sum(-1, dtype=np.float32)
        M1 = m1.max(-1, keepdims=True)
        a = np.where(np.isfinite(m1), np.exp((m1 - M1).astype(np.float32)), np.float32(0))
        dm = np.where(np.isfinite(m1), m1 - M1, np.float32(0)).astype(np.float32)
        S = (s1 * a).sum(-1, dtype=np.float32)
        U = ((u1 + dm * s1) * a).sum(-1, dtype=np.float32)
    H32 = np.log(S) - U / S
    assert (np.abs(H32.astype(np.float64) - H) <= 0.05 * tol).all(), (np.abs(H32 - H) / tol).max()


# ---- the kernels ----------------------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def first_case(V):
    """(H [B] float32 numpy of the top-k / top-p case): the bits every other case must reproduce."""
    lg = torch.from_numpy(inputs(V)).to(DEV)
    args, kw = device_args(V, CASES[0])
    return ops.sample_ent(lg, *args, seed=77, step=0, **kw)[2][:, 0].cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("V", SIZES)
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_entropy_against_float64_and_everything_else_is_sample_guided(V, case):
    """ent_out against float64 at rtol 1e-5, atol 1e-5; the same bits as the top-k / top-p case for every row (the filter, the penalty, the guide and the sampling
    path do not enter); ids, logp_out, seen and state bit-equal to ops.sample_guided on the same arguments."""
    x = inputs(V)
    lg = torch.from_numpy(x).to(DEV)
    args, kw = device_args(V, case)
    args2, kw2 = device_args(V, case)
    ids, lp, ent = ops.sample_ent(lg, *args, seed=77, step=0, **kw)
    ids2, lp2 = ops.sample_guided(lg, *args2, seed=77, step=0, **kw2)
    assert torch.equal(ids, ids2) and torch.equal(lp, lp2)
    for name in ("seen", "state"):
        if name in kw:
            assert torch.equal(kw[name], kw2[name]), name
    assert tuple(ent.shape) == (B, 1) and ent.dtype == F32
    close(ent[:, 0].cpu().numpy(), entropy64(x), f"V={V} {case[0]}")
    assert np.array_equal(ent[:, 0].cpu().numpy(), first_case(V)), "the entropy depends on something the filter does"
    assert torch.equal(lg, torch.from_numpy(x).to(DEV)), "the logits were written"


@pytest.mark.gpu
@pytest.mark.parametrize("V", SIZES)
def test_a_suppressed_token_counts_in_the_entropy(V):
    """suppress_token = the row's argmax, one call per gaussian-type row: the entropy keeps the bits of the unsuppressed call in every row (the suppressed logit counts, as
    in (m1, s1)), the pick avoids the token, and ids / logp_out are those of ops.sample_guided with the same suppress_token."""
    x = inputs(V)
    lg = torch.from_numpy(x).to(DEV)
    for path in ((T, 50, 0.9), (T, 0, 1.0), (0.0, 1, 1.0)):
        for r in RANDN_ROWS:
            sup = int(x[r].argmax())
            ids, lp, ent = ops.sample_ent(lg, *path, seed=77, step=0, suppress_token=sup)
            ids2, lp2 = ops.sample_guided(lg, *path, seed=77, step=0, suppress_token=sup)
            assert torch.equal(ids, ids2) and torch.equal(lp, lp2) and int(ids[r]) != sup
            assert np.array_equal(ent[:, 0].cpu().numpy(), first_case(V)), (path, r)
    close(first_case(V), entropy64(x), f"V={V} suppressed")


@pytest.mark.gpu
def test_step_ptr_selects_the_column_and_a_column_outside_is_left_alone():
    """The column rule of logp_out: column = *step_ptr (else step); a step >= ent_cols writes nothing.  The buffer is [B, 3] with row stride 5 inside a larger
    allocation of sentinels, 8 in front and behind."""
    V = SIZES[1]
    x = inputs(V)
    lg = torch.from_numpy(x).to(DEV)
    want = first_case(V)
    for path in ((T, 50, 0.9), (T, 0, 1.0), (0.0, 1, 1.0)):
        for step, use_ptr in ((0, False), (1, True), (2, False), (3, True), (7, False), (1 << 20, True)):
            whole = torch.full((16 + B * 5,), SENT, dtype=F32, device=DEV)
            ent = whole[8: 8 + B * 5].view(B, 5)[:, :3]
            lp = torch.full((B, 3), SENT, dtype=F32, device=DEV)
            sp = torch.tensor([step], dtype=torch.int32, device=DEV) if use_ptr else None
            ids, _, e2 = ops.sample_ent(lg, *path, seed=77, step=0 if use_ptr else step, step_ptr=sp, logp_out=lp, ent_out=ent)
            ids2, lp2 = ops.sample_guided(lg, *path, seed=77, step=0 if use_ptr else step, step_ptr=sp, logp_out=torch.full((B, 3), SENT, dtype=F32, device=DEV))
            assert e2 is ent and torch.equal(ids, ids2) and torch.equal(lp, lp2)
            got = whole.cpu().numpy()
            exp = np.full(16 + B * 5, SENT, dtype=np.float32)
            if step < 3:
                exp[8: 8 + B * 5].reshape(B, 5)[:, step] = want
            assert np.array_equal(got, exp), (path, step, use_ptr)


@pytest.mark.gpu
@pytest.mark.parametrize("case", [CASES[0], CASES[4], CASES[5]], ids=lambda c: c[0])
def test_without_ent_out_the_call_is_sample_guided(case):
    V = SIZES[1]
    lg = torch.from_numpy(inputs(V)).to(DEV)
    args, kw = device_args(V, case)
    args2, kw2 = device_args(V, case)
    ids, lp, ent = ops.sample_ent(lg, *args, seed=5, step=0, want_ent=False, **kw)
    ids2, lp2 = ops.sample_guided(lg, *args2, seed=5, step=0, **kw2)
    assert ent is None and torch.equal(ids, ids2) and torch.equal(lp, lp2)
    for name in ("seen", "state"):
        if name in kw:
            assert torch.equal(kw[name], kw2[name]), name
