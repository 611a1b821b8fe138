"""The attention family (csrc/attn.hip, csrc/attn_decode.hip) against float64, on inputs built so that a mask or page bug cannot hide.

Every output element is held to  |got - ref64| <= 2^-6 * E,  where E is the same computation with absolute values (E_o = P |V|, E_dv = sum_heads P^T |dO|,
E_dq = scale A |K|, E_dk = sum_heads scale A^T |Q| with A = P o (|dP| + delta_abs), delta_abs_i = sum_d |o_id dO_id|).  The constant is derived, not tuned: the
kernels round P, dS and every output to bf16 with round-to-nearest (2^-8 relative each), delta is formed from the bf16-rounded o, everything else is fp32 -- at most
2 * 2^-8 * E for o and dv, 3 * 2^-8 * E for dq and dk; 2^-6 = 4 * 2^-8 leaves the rest to v_exp_f32 and the fp32 summation order.  The log-sum-exp is fp32 end to
end: |got - ref64| <= 1e-4 * max(1, |ref|), and exactly -inf where no key is visible.

The inputs: N(0,1) everywhere, except (a) NEEDLE keys at the boundary positions of a case (K = 0.6 q of the first q head of the kv group, V = 3: a softmax weight
>= 0.02, asserted), (b) finite POISON wherever nothing may be read (unused slots of a used page, the page that block-table entries past the needed ones point to,
K/V/dO rows outside every segment: K = 4 q, V = 100), and (c) q rows copied so that key i + 1 is a needle for row i too.

The CPU part proves the GPU part's sensitivity: a torch emulation of the kernels' arithmetic (float64 with their bf16 rounding points, 64-key tiles, 32-key pages
split over the waves and merged) stays inside the bounds on every input set the GPU tests use, and every fault model -- applied to the float64 reference on the same
inputs -- exceeds the bound at least 4 x at the rows it was designed for."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import iadr1_amd  # noqa: E402,F401
from iadr1_amd import ops  # noqa: E402
from test_hip_kernels import ATTN_CASES, PREFIX_CASES  # noqa: E402

DEV = "cuda"
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
BOUND = 2.0 ** -6          # x E, every bf16 output
TINY = 1e-30               # denormal guard
LSE_RTOL = 1e-4            # x max(1, |ref|)
FAULT_FACTOR = 4.0
NEEDLE_W = 0.02
PAGE = 32


# ======================================================================================================================================================
# helpers: float64 reference with its error scale, the emulation of the kernels' arithmetic
# ======================================================================================================================================================

def bfr(x):
    """round to bf16 (nearest even), back in float64"""
    return x.to(BF).to(F64)


def _expand(K, Hq, kvmap=None):
    Hkv = K.shape[0]
    if kvmap is None:
        return K.repeat_interleave(Hq // Hkv, 0)
    return K[kvmap]


def attend(Q, K, V, vis, scale, dO=None, kvmap=None):
    """Float64 attention of Q [Hq, nq, D] over K, V [Hkv, nk, D] with the visibility mask vis [nq, nk] (GQA: q head h reads kv head h // group, or kvmap[h]).
    Returns o, lse, P and the error scale E_o; with dO also dq, E_dq [Hq, nq, D] and this call's contributions dk, E_dk, dv, E_dv [Hkv, nk, D] (closed formulas)."""
    Hq, nq, D = Q.shape
    Hkv = K.shape[0]
    if K.shape[1] == 0:         # no key at all: one invisible key keeps the reductions defined
        K, V, vis = torch.zeros_like(Q[:Hkv, :1]), torch.zeros_like(Q[:Hkv, :1]), torch.zeros(nq, 1, dtype=torch.bool, device=Q.device)
    Kx, Vx = _expand(K, Hq, kvmap), _expand(V, Hq, kvmap)
    S = (Q @ Kx.transpose(1, 2)) * scale
    S = S.masked_fill(~vis, float("-inf"))
    lse = torch.logsumexp(S, -1)
    P = torch.exp(S - torch.where(torch.isinf(lse), torch.zeros_like(lse), lse)[..., None])
    r = {"o": P @ Vx, "lse": lse, "P": P, "E_o": P @ Vx.abs()}
    if dO is not None:
        dP = dO @ Vx.transpose(1, 2)
        delta = (r["o"] * dO).sum(-1, keepdim=True)
        dS = P * (dP - delta)
        A = P * (dP.abs() + (r["o"] * dO).abs().sum(-1, keepdim=True))
        grp = lambda t: t.view(Hkv, Hq // Hkv, *t.shape[1:]).sum(1)
        r.update(dq=scale * (dS @ Kx), E_dq=scale * (A @ Kx.abs()), dk=grp(scale * (dS.transpose(1, 2) @ Q)), E_dk=grp(scale * (A.transpose(1, 2) @ Q.abs())),
                 dv=grp(P.transpose(1, 2) @ dO), E_dv=grp(P.transpose(1, 2) @ dO.abs()))
    return r


def emu_stream(Q, Kx, Vx, vis, scale, tiles, state=None):
    """One online-softmax stream of the kernels over the key tiles [(a, b), ...]: float64 arithmetic, P rounded to bf16 where it enters P.V, the row sum
    from the unrounded p.  state = (m, l, acc)."""
    Hq, nq, D = Q.shape
    if state is None:
        state = (torch.full((Hq, nq), float("-inf"), dtype=F64, device=Q.device), torch.zeros(Hq, nq, dtype=F64, device=Q.device),
                 torch.zeros(Hq, nq, D, dtype=F64, device=Q.device))
    m, l, acc = state
    for a, b in tiles:
        s = ((Q @ Kx[:, a:b].transpose(1, 2)) * scale).masked_fill(~vis[..., a:b], float("-inf"))
        mn = torch.maximum(m, s.amax(-1))
        dead = torch.isinf(mn)
        mref = torch.where(dead, torch.zeros_like(mn), mn)
        alpha = torch.where(dead, torch.ones_like(mn), torch.exp(m - mref))
        p = torch.exp(s - mref[..., None])
        l = l * alpha + p.sum(-1)
        acc = acc * alpha[..., None] + bfr(p) @ Vx[:, a:b]
        m = mn
    return m, l, acc


def emu_merge(states):
    """Merge of partial online-softmax states (WaveRed::get, the chunk merge and the group kernel's phase 2 are this sum in different groupings)."""
    M = torch.stack([s[0] for s in states]).amax(0)
    num, den = 0.0, 0.0
    for m, l, acc in states:
        f = torch.where(torch.isinf(m), torch.zeros_like(m), torch.exp(m - torch.where(torch.isinf(M), torch.zeros_like(M), M)))
        num, den = num + f[..., None] * acc, den + f * l
    return M, den, num


def emu_finish(m, l, acc):
    """o rounded to bf16, lse stored as fp32"""
    live = l > 0
    o = bfr(torch.where(live[..., None], acc / torch.where(live, l, torch.ones_like(l))[..., None], torch.zeros_like(acc)))
    lse = torch.where(live, m + torch.log(torch.where(live, l, torch.ones_like(l))), torch.full_like(m, float("-inf")))
    return o, lse.to(F32).to(F64)


def emu_attend(Q, K, V, vis, scale, tiles, dO=None):
    """The training kernels' arithmetic: forward over 64-key tiles; backward with p = exp(s - lse32), delta from the bf16 o, dS and P rounded to bf16 where they enter
    the second GEMMs, dq rounded to bf16 (dk / dv are rounded by the caller, after every contribution is in)."""
    Hq, nq, D = Q.shape
    Hkv = K.shape[0]
    Kx, Vx = _expand(K, Hq), _expand(V, Hq)
    o, lse = emu_finish(*emu_stream(Q, Kx, Vx, vis, scale, tiles))
    r = {"o": o, "lse": lse}
    if dO is not None:
        S = ((Q @ Kx.transpose(1, 2)) * scale).masked_fill(~vis, float("-inf"))
        P = torch.exp(S - torch.where(torch.isinf(lse), torch.zeros_like(lse), lse)[..., None])
        P = torch.where(vis, P, torch.zeros_like(P))
        delta = (o * dO).sum(-1, keepdim=True)
        dS = bfr(P * (dO @ Vx.transpose(1, 2) - delta))
        grp = lambda t: t.view(Hkv, Hq // Hkv, *t.shape[1:]).sum(1)
        r.update(dq=bfr(scale * (dS @ Kx)), dk=grp(scale * (dS.transpose(1, 2) @ Q)), dv=grp(bfr(P).transpose(1, 2) @ dO))
    return r


def ratio(got, ref, E):
    """|got - ref| in units of the bound 2^-6 E"""
    return (got.double() - ref).abs() / (BOUND * E + TINY)


def check_bound(what, got, ref, E, row_names=None):
    """got, ref, E: [rows, heads, D].  Asserts |got - ref| <= 2^-6 E everywhere; the failure lists the worst (row, head) pairs with err / E.  Returns max err / (2^-6 E)."""
    rt = ratio(got, ref, E)
    worst = rt.amax(-1)
    mx = float(worst.max()) if worst.numel() else 0.0
    if mx > 1.0:
        bad = (worst > 1.0).nonzero().cpu().tolist()
        flat = sorted(bad, key=lambda ij: -float(worst[ij[0], ij[1]]))[:8]
        lines = []
        for i, h in flat:
            d = int(rt[i, h].argmax())
            lines.append(f"row {row_names[i] if row_names is not None else i} head {h} dim {d}: got {float(got[i, h, d]):.6g} ref {float(ref[i, h, d]):.6g} "
                         f"err/E {float(worst[i, h]) * BOUND:.4g} = {float(worst[i, h]):.2f} x 2^-6")
        raise AssertionError(f"{what}: {len(bad)} of {worst.numel()} (row, head) pairs beyond 2^-6 E\n  " + "\n  ".join(lines))
    return mx


def check_lse(what, got, ref, row_names=None):
    """got, ref: [heads, rows].  -inf exactly where the reference is -inf, else |got - ref| <= 1e-4 max(1, |ref|).  Returns the largest error in units of the bound."""
    got, ref = got.double(), ref.double()
    dead = torch.isinf(ref)
    assert bool((got[dead] == ref[dead]).all()), f"{what}: rows with no visible key must hold exactly -inf"
    err = torch.where(dead, torch.zeros_like(ref), (got - ref).abs() / (LSE_RTOL * ref.abs().clamp(min=1.0)))
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
    mx = float(err.max()) if err.numel() else 0.0
    if mx > 1.0:
        bad = (err > 1.0).nonzero().cpu().tolist()[:8]
        lines = [f"head {h} row {row_names[i] if row_names is not None else i}: got {float(got[h, i]):.8g} ref {float(ref[h, i]):.8g}" for h, i in bad]
        raise AssertionError(f"{what}: log-sum-exp beyond 1e-4 max(1, |ref|)\n  " + "\n  ".join(lines))
    return mx


# ======================================================================================================================================================
# segment (training) attention: input sets, the float64 reference over a layout, fault models
# ======================================================================================================================================================

def needle_v(D, code):
    """V of a needle: 3 in every dim, signed by the Walsh pattern `code` (bit b set: the sign flips with bit b of d).  Needles that share their key (twins: the
    needles of one decode sequence, a prompt's last key and its child's first, the last key of a segment and the first of the next) get different patterns:
    with one V they would cover for each other, with opposite V their sum would vanish like an empty page."""
    d = torch.arange(D)
    sgn = torch.ones(D)
    for b in range(4):
        if (code >> b) & 1:
            sgn = sgn * (1.0 - 2.0 * ((d >> b) & 1))
    return 3.0 * sgn


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def make_layout(D, Hq, Hkv, causal, segs, parent=None, seed=1, name=""):
    """One input set: q | k | v rows [T, (Hq + 2 Hkv) D] and dO [T, Hq D] in bf16 (CPU) + the segment list.  parent[i]: index of segment i's prompt, or None.
    Needle rows (diagonal key = 0.6 q of the group's first head, |V| = 3, needle_v): 63, 64, 127, 128, slen - 1 of every segment, and the first own row behind a prefix.
    Links make the NEXT key a needle as well (q of the first head copied): row j - 1 <- needle row j; the last row of a segment <- the first row of the segment that
    follows it directly; a child's first row <- its prompt's last row.  Rows outside every segment are poison: K = 4 q of the anchor row (the first row of the
    segment that starts right behind a gap of >= 2 rows for the gap's last row, else the last row of the segment before; the first segment's row 0 in front of
    everything), V = 100, dO = 100."""
    nseg = len(segs)
    parent = parent or [None] * nseg
    T = max(e for _, e in segs) + 5
    grp = Hq // Hkv
    g = _gen(seed)
    q, k, v = torch.randn(T, Hq, D, generator=g), torch.randn(T, Hkv, D, generator=g), torch.randn(T, Hkv, D, generator=g)
    do = torch.randn(T, Hq, D, generator=_gen(seed + 1))
    q, k, v, do = (t.to(BF).float() for t in (q, k, v, do))
    h0 = torch.arange(Hkv) * grp
    owner = np.full(T, -1)
    for i, (s, e) in enumerate(segs):
        assert e > s and (owner[s:e] == -1).all()
        owner[s:e] = i
    needles = []
    for i, (s, e) in enumerate(segs):
        n = e - s
        js = {j for j in (63, 64, 127, 128, n - 1) if j < n}
        if parent[i] is not None:
            js |= {0, n - 1}
        needles.append(sorted(js))
    plain = all(p is None for p in parent)
    links = set()
    for i, (s, e) in enumerate(segs):
        links |= {s + j for j in needles[i] if j >= 1 and j - 1 not in needles[i]}      # row r - 1 <- row r (not onto a needle row: twins would cover for each other)
        if plain and s >= 1 and owner[s - 1] >= 0:
            links.add(s)
    for r in sorted(links, reverse=True):
        q[r - 1, h0] = q[r, h0]
    for i, (s, e) in enumerate(segs):
        if parent[i] is not None:
            q[s, h0] = q[segs[parent[i]][1] - 1, h0]
            if 1 in needles[i]:
                q[s + 1, h0] = q[s, h0]
    for i, (s, e) in enumerate(segs):
        for j in needles[i]:
            k[s + j] = (0.6 * q[s + j, h0]).to(BF).float()
            v[s + j] = needle_v(D, 1 if (parent[i] is not None and j == 0) else (2 if (plain and j == e - s - 1 and i % 2) else 0))
    first_start = min(s for s, _ in segs)
    anchors = {}
    for r in range(T):
        if owner[r] >= 0:
            continue
        before = [e for _, e in segs if e <= r]
        starts_next = any(s == r + 1 for s, _ in segs)
        if not before:
            a = first_start
        elif starts_next and r >= 1 and owner[r - 1] < 0:
            a = r + 1
        else:
            a = max(before) - 1
        anchors[r] = a
        k[r] = 4.0 * q[a, h0]
        v[r] = 100.0
        do[r] = 100.0
    qkv = torch.cat([q.reshape(T, -1), k.reshape(T, -1), v.reshape(T, -1)], 1).to(BF)
    return {"name": name, "D": D, "Hq": Hq, "Hkv": Hkv, "causal": causal, "scale": D ** -0.5, "segs": list(segs), "parent": parent, "T": T, "qkv": qkv,
            "do": do.reshape(T, -1).to(BF), "needles": needles, "owner": owner, "anchors": anchors, "h0": h0}


def prefix_table(L):
    """seg_prefix rows {prefix_start, prefix_len, child_first, child_count} of a layout (children of a prompt are consecutive in the segment list)"""
    out = []
    for i, (s, e) in enumerate(L["segs"]):
        kids = [j for j, p in enumerate(L["parent"]) if p == i]
        if L["parent"][i] is not None:
            ps, pe = L["segs"][L["parent"][i]]
            out.append([ps, pe - ps, 0, 0])
        else:
            assert not kids or kids == list(range(kids[0], kids[0] + len(kids)))
            out.append([0, 0, kids[0] if kids else 0, len(kids)])
    return out


def split(L, dev):
    """q, k, v, dO as float64 [T, heads, D] on `dev`"""
    D, Hq, Hkv, T = L["D"], L["Hq"], L["Hkv"], L["T"]
    x = L["qkv"].to(dev).double()
    return (x[:, : Hq * D].reshape(T, Hq, D), x[:, Hq * D: (Hq + Hkv) * D].reshape(T, Hkv, D), x[:, (Hq + Hkv) * D:].reshape(T, Hkv, D),
            L["do"].to(dev).double().reshape(T, Hq, D))


def seg_keys(L, i, dev, fault=None):
    """(key rows, visibility [nq, nk], number of prefix keys) of segment i, the fault model applied"""
    s, e = L["segs"][i]
    n = e - s
    own = torch.arange(s, e, device=dev)
    pre = torch.arange(0, 0, device=dev)
    p = L["parent"][i]
    if p is not None:
        pre = torch.arange(*L["segs"][p], device=dev)
    if fault == "other_prefix" and p is not None:
        others = [j for j, pp in enumerate(L["parent"]) if pp is None and j != p and any(x == j for x in L["parent"])]
        if others:
            pre = torch.arange(*L["segs"][others[0]], device=dev)
    ones = lambda a, b: torch.ones(a, b, dtype=torch.bool, device=dev)
    diag = {"strict": -1, "permissive": 1}.get(fault, 0)
    vo = ones(n, n).tril(diag) if L["causal"] else ones(n, n)
    vp = ones(n, len(pre))
    if fault == "prefix_causal":
        vp = vp.tril(0)
    krows, vis = torch.cat([pre, own]), torch.cat([vp, vo], 1)
    if fault == "before_start":
        extra = torch.arange(max(0, s - 32), s, device=dev)
        krows, vis = torch.cat([extra, krows]), torch.cat([ones(n, len(extra)), vis], 1)
    if fault == "past_end":
        extra = torch.arange(e, min(L["T"], e + 8), device=dev)
        extra = extra[torch.as_tensor(L["owner"][extra.cpu().numpy()] < 0, device=dev)] if len(extra) else extra
        krows, vis = torch.cat([krows, extra]), torch.cat([vis, ones(n, len(extra))], 1)
    return krows, vis, len(pre)


def run_layout(L, dev="cpu", emu=False, fault=None, backward=True):
    """Float64 reference (or the emulation) of a whole layout: o, lse, dq, dk, dv [+ E_*] as [T, heads, D] / [Hq, T]; rows outside every segment stay 0 / -inf."""
    D, Hq, Hkv, T, sc = L["D"], L["Hq"], L["Hkv"], L["T"], L["scale"]
    q, k, v, do = split(L, dev)
    z = lambda h: torch.zeros(T, h, D, dtype=F64, device=dev)
    R = {"o": z(Hq), "lse": torch.full((Hq, T), float("-inf"), dtype=F64, device=dev), "dq": z(Hq), "dk": z(Hkv), "dv": z(Hkv)}
    if not emu:
        R.update(E_o=z(Hq), E_dq=z(Hq), E_dk=z(Hkv), E_dv=z(Hkv), needle_w={})
    for i, (s, e) in enumerate(L["segs"]):
        krows, vis, npre = seg_keys(L, i, dev, fault)
        Q, K, V = q[s:e].transpose(0, 1), k[krows].transpose(0, 1), v[krows].transpose(0, 1)
        dO = do[s:e].transpose(0, 1) if backward else None
        if emu:
            tiles = [(a, min(a + 64, npre)) for a in range(0, npre, 64)] + [(a, min(a + 64, len(krows))) for a in range(npre, len(krows), 64)]
            r = emu_attend(Q, K, V, vis, sc, tiles, dO)
        else:
            r = attend(Q, K, V, vis, sc, dO)
            if fault is None:
                for j in L["needles"][i]:
                    R["needle_w"][(i, j)] = float(r["P"][L["h0"].to(dev), j, npre + j].min())
        R["o"][s:e], R["lse"][:, s:e] = r["o"].transpose(0, 1), r["lse"]
        if not emu:
            R["E_o"][s:e] = r["E_o"].transpose(0, 1)
        if backward:
            R["dq"][s:e] = r["dq"].transpose(0, 1)
            R["dk"].index_add_(0, krows, r["dk"].transpose(0, 1))
            R["dv"].index_add_(0, krows, r["dv"].transpose(0, 1))
            if not emu:
                R["E_dq"][s:e] = r["E_dq"].transpose(0, 1)
                R["E_dk"].index_add_(0, krows, r["E_dk"].transpose(0, 1))
                R["E_dv"].index_add_(0, krows, r["E_dv"].transpose(0, 1))
    if emu and backward:
        R["dk"], R["dv"] = bfr(R["dk"]), bfr(R["dv"])
    return R


def inside_rows(L):
    return torch.as_tensor(np.nonzero(L["owner"] >= 0)[0])


# ---- the input sets of the GPU tests --------------------------------------------------------------------------------------------------------------

def _ragged(lengths, gaps, start):
    segs, r = [], start
    for n, gp in zip(lengths, gaps):
        segs.append((r, r + n))
        r += n + gp
    return segs


EDGE_LENGTHS = [1, 2, 63, 64, 65, 127, 128, 129, 256, 257]
EDGE_GAPS = [3, 0, 2, 0, 0, 7, 0, 5, 0, 2]         # gaps are 0 (neighbours) or >= 2 (poison anchored to both sides)


@functools.lru_cache(maxsize=None)
def plain_layouts():
    out = [make_layout(D, Hq, Hkv, causal, segs, seed=11 + i, name=f"ATTN_CASES[{i}]") for i, (D, Hq, Hkv, causal, segs) in enumerate(ATTN_CASES)]
    out.append(make_layout(128, 4, 2, True, _ragged(EDGE_LENGTHS, EDGE_GAPS, 3), seed=41, name="edge lengths 4:2 causal"))
    out.append(make_layout(128, 28, 4, True, _ragged(EDGE_LENGTHS[::-1], EDGE_GAPS, 5), seed=42, name="edge lengths 28:4 causal"))
    out.append(make_layout(80, 2, 2, False, _ragged(EDGE_LENGTHS, EDGE_GAPS, 3), seed=43, name="edge lengths D=80 non-causal"))
    return out


def _prefix_layout(Hq, Hkv, prompts, comps, ordered, seed, name):
    """ordered: prompts first, then every child (the launch hint nseg_head / max_seqlen_tail is on); else prompt, its children, next prompt, ... (hint off)"""
    segs, parent = [], []
    if ordered:
        segs, parent = list(prompts), [None] * len(prompts)
        for p, cs in enumerate(comps):
            segs += list(cs)
            parent += [p] * len(cs)
    else:
        for pr, cs in zip(prompts, comps):
            at = len(segs)
            segs += [pr] + list(cs)
            parent += [None] + [at] * len(cs)
    return make_layout(128, Hq, Hkv, True, segs, parent=parent, seed=seed, name=name)


def _edge_prefix(start):
    """prompts of 1, 63, 64, 65, 512 tokens, children that include length 1; gaps of 0 or >= 2 rows"""
    plens, kids = [1, 63, 64, 65, 512], [[1, 40], [64, 1], [65], [1, 33, 129], [17, 1, 256]]
    r, prompts, comps = start, [], []
    for n in plens:
        prompts.append((r, r + n))
        r += n + (2 if n == 64 else 0)
    r += 3
    for cs in kids:
        row = []
        for n in cs:
            row.append((r, r + n))
            r += n + (4 if n == 1 else 0)
        comps.append(row)
    return prompts, comps


@functools.lru_cache(maxsize=None)
def prefix_layouts():
    out = [_prefix_layout(Hq, Hkv, pr, cs, True, 21 + i, f"PREFIX_CASES[{i}]") for i, (Hq, Hkv, pr, cs) in enumerate(PREFIX_CASES)]
    pr, cs = _edge_prefix(2)
    out.append(_prefix_layout(16, 2, pr, cs, True, 51, "edge prefixes 16:2, prompts first (hint on)"))
    out.append(_prefix_layout(4, 2, pr, cs, False, 52, "edge prefixes 4:2, prompts between their children (hint off)"))
    out.append(_prefix_layout(28, 4, pr[:4], cs[:4], False, 53, "edge prefixes 28:4, hint off"))
    return out


# ---- fault models of the training kernels: (name, designated query rows) -----------------------------------------------------------------------------

def designated(L, fault):
    """Flat query rows where the fault must show (every row is checked at the first q head of each kv group)"""
    rows = []
    for i, (s, e) in enumerate(L["segs"]):
        n, p = e - s, L["parent"][i]
        if fault == "strict" and L["causal"]:
            rows += [s + j for j in L["needles"][i]]
        if fault == "permissive" and L["causal"]:
            rows += [s + j - 1 for j in L["needles"][i] if j >= 1 and j - 1 not in L["needles"][i]]
        if fault == "before_start" and all(pp is None for pp in L["parent"]) and s >= 1:
            if L["owner"][s - 1] >= 0 or L["anchors"].get(s - 1) == s:
                rows.append(s)
        if fault == "past_end" and e < L["T"] and L["owner"][e] < 0 and L["anchors"][e] == e - 1:
            rows.append(e - 1)
        if fault == "prefix_causal" and p is not None and L["segs"][p][1] - L["segs"][p][0] >= 2:
            rows.append(s)
        if fault == "other_prefix" and p is not None and sum(1 for j, pp in enumerate(L["parent"]) if pp is None and j in L["parent"]) >= 2:
            rows.append(s)
    return rows


TRAIN_FAULTS = ["strict", "permissive", "before_start", "prefix_causal", "other_prefix", "past_end"]


# ======================================================================================================================================================
# paged decode attention: input sets, reference, emulation, fault models
# ======================================================================================================================================================

DECODE_LENS = [0, 1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 517, 767, 3185]      # pages: 0 .. 100 -- below, at and above the 16 waves of the kernel
DECODE_GEOMS = [(16, 2), (28, 4), (32, 8), (32, 32), (2, 1)]
GROUP_EXTRA = [0, 1, 30, 31, 32, 63, 100, 255]
GROUP_CASES = [  # Hq, Hkv, G, prompt lengths: k * 32 exactly, shorter than a page (no shared page), 3184
    (16, 2, 8, [512, 31]),
    (32, 8, 4, [3184, 64]),
    (28, 4, 3, [100, 7, 96]),
    (2, 1, 2, [32, 7, 3184]),
    (32, 32, 2, [832, 20]),
]
GROUP_CHUNKS = [1, 2, 5, 33]        # 33 is more than the shared pages of every prompt but the 3184-token one


def make_decode(Hq, Hkv, ctx, G=1, prompts=None, seed=3):
    """q [B, Hq D] and per sequence its keys / values [n, Hkv, D] + 64 poison rows (K = 4 q of the group's first head, V = 100) that fill the unused slots of its
    last page and the page its spare block-table entries point to.  Needles (|V| = 3, needle_v) at key 0, the first key of the last page and key n - 1.  G > 1: the sequences of a group
    share their first prompts[b // G] keys and the q of the first head of every kv group (so that a shared key is a needle for all of them)."""
    D, B, grp = 128, len(ctx), Hq // Hkv
    g = _gen(seed)
    q = torch.randn(B, Hq, D, generator=g).to(BF).float()
    h0 = torch.arange(Hkv) * grp
    if G > 1:
        for b in range(B):
            q[b, h0] = q[b // G * G, h0]
    seqs, shared_kv = [], {}
    for b, n in enumerate(ctx):
        K, V = torch.randn(n, Hkv, D, generator=g).to(BF).float(), torch.randn(n, Hkv, D, generator=g).to(BF).float()
        if G > 1:
            pl = prompts[b // G]
            if b % G == 0:
                shared_kv[b // G] = (K[:pl].clone(), V[:pl].clone())
            K[:pl], V[:pl] = shared_kv[b // G]
        npage = (n + PAGE - 1) // PAGE
        pos = sorted({0, PAGE * (npage - 1), n - 1}) if n > 0 else []
        for i_, p_ in enumerate(pos):
            K[p_] = (0.6 * q[b, h0]).to(BF).float()
            V[p_] = torch.stack([needle_v(D, i_ + 4 * (kvh & 1)) for kvh in range(Hkv)])
        Kp, Vp = (4.0 * q[b, h0])[None].expand(2 * PAGE, Hkv, D).clone(), torch.full((2 * PAGE, Hkv, D), 100.0)
        seqs.append({"n": n, "K": K, "V": V, "Kp": Kp, "Vp": Vp, "needles": pos, "npage": npage})
    return {"Hq": Hq, "Hkv": Hkv, "D": D, "B": B, "G": G, "prompts": prompts, "q": q, "seqs": seqs, "h0": h0, "scale": D ** -0.5, "ctx": list(ctx)}


def full_view(s):
    """what the sequence's block table addresses: its keys, the poison in the rest of its last page, one more (poison) page"""
    pad = s["npage"] * PAGE - s["n"] + PAGE
    return torch.cat([s["K"], s["Kp"][:pad]]), torch.cat([s["V"], s["Vp"][:pad]])


def decode_ref(dd, b, dev="cpu", fault=None):
    """float64 reference of sequence b (attend() with one query row), the fault model applied.  Returns None where the fault does not apply."""
    s = dd["seqs"][b]
    n, npage = s["n"], s["npage"]
    Kf, Vf = (t.to(dev).double() for t in full_view(s))
    Q = dd["q"][b].to(dev).double()[:, None, :]
    idx = torch.arange(n, device=dev)
    kvmap = None
    if fault == "ctx_minus_1":
        if n < 1:
            return None
        idx = idx[:-1]
    elif fault == "ctx_plus_1":
        idx = torch.arange(n + 1, device=dev)
    elif fault == "tail_unmasked":
        if n % PAGE == 0:
            return None
        idx = torch.arange(npage * PAGE, device=dev)
    elif fault in ("skip_first_page", "skip_last_page"):
        if n < 1:
            return None
        pg = 0 if fault == "skip_first_page" else npage - 1
        idx = idx[(idx // PAGE) != pg]
    elif fault == "extra_table_entry":
        idx = torch.cat([idx, torch.arange(npage * PAGE, (npage + 1) * PAGE, device=dev)])
    elif fault == "v_swapped":
        if n < 1:
            return None
        Vf = Vf.clone()
        Vf[[0, 1]] = Vf[[1, 0]]          # key 1 is a real key, or (n = 1) a poison slot of the same page
    elif fault == "wrong_kv_head":
        if dd["Hkv"] < 2 or n < 1:
            return None
        kvmap = ((torch.arange(dd["Hq"], device=dev) // (dd["Hq"] // dd["Hkv"])) + 1) % dd["Hkv"]
    K, V = Kf[idx].transpose(0, 1), Vf[idx].transpose(0, 1)
    vis = torch.ones(1, len(idx), dtype=torch.bool, device=dev)
    return attend(Q, K, V, vis, dd["scale"], kvmap=kvmap)


DECODE_FAULTS = ["ctx_minus_1", "ctx_plus_1", "tail_unmasked", "skip_first_page", "skip_last_page", "extra_table_entry", "v_swapped", "wrong_kv_head"]


def decode_emu(dd, b, streams, dev="cpu"):
    """The decode kernels' arithmetic for sequence b: every stream (a list of page indices) is one wave's online softmax over its 32-key pages, the partial
    states are merged, o is rounded to bf16."""
    s = dd["seqs"][b]
    n = s["n"]
    Kf, Vf = (t.to(dev).double().transpose(0, 1) for t in full_view(s))
    Q = dd["q"][b].to(dev).double()[:, None, :]
    Kx, Vx = _expand(Kf, dd["Hq"]), _expand(Vf, dd["Hq"])
    vis = (torch.arange(Kf.shape[1], device=dev) < n)[None, :]
    states = [emu_stream(Q, Kx, Vx, vis, dd["scale"], [(pg * PAGE, (pg + 1) * PAGE) for pg in st]) for st in streams]
    M, den, num = emu_merge(states)
    return emu_finish(M, den, num)


def wave_streams(npage, waves=16, first=0):
    return [list(range(first + w, npage, waves)) for w in range(waves)]


def group_streams(npage, ns, chunks):
    """attn_decode_group: the shared pages [0, ns) in `chunks` ranges of ceil(ns / chunks) pages, each walked by 8 waves; the private pages by one wave"""
    per = (ns + chunks - 1) // chunks if chunks > 1 else ns
    out = []
    for c in range(chunks):
        p0, p1 = c * per, min(ns, c * per + per)
        out += [list(range(p0 + w, p1, 8)) for w in range(8)]
    return out + [list(range(ns, npage))]


@functools.lru_cache(maxsize=None)
def decode_sets():
    return [make_decode(Hq, Hkv, DECODE_LENS, seed=60 + i) for i, (Hq, Hkv) in enumerate(DECODE_GEOMS)]


@functools.lru_cache(maxsize=None)
def group_sets():
    out = []
    for i, (Hq, Hkv, G, prompts) in enumerate(GROUP_CASES):
        ctx = [prompts[b // G] + GROUP_EXTRA[(b + b // G) % len(GROUP_EXTRA)] + 1 for b in range(len(prompts) * G)]
        out.append(make_decode(Hq, Hkv, ctx, G=G, prompts=prompts, seed=80 + i))
    return out


def paged_cache(dd, dev, seed=0):
    """The physical cache of an input set, written through ops.kv_store: permuted page ids, shared prompt pages (G > 1) written once, the unused slots of every last
    page and one page per sequence -- the target of ALL its spare block-table entries -- filled with poison.  Returns kcache, vcache, block table, shared pages."""
    Hkv, D, B, G = dd["Hkv"], dd["D"], dd["B"], dd["G"]
    nsh = [(dd["prompts"][b // G] // PAGE if G > 1 else 0) for b in range(B)]
    logical, nxt = [], 0
    for b, s in enumerate(dd["seqs"]):
        if G > 1 and b % G:
            pages = logical[b // G * G][: nsh[b]]
        else:
            pages = list(range(nxt, nxt + nsh[b]))
            nxt += nsh[b]
        priv = s["npage"] - nsh[b] + 1          # + its poison page
        logical.append(pages + list(range(nxt, nxt + priv)))
        nxt += priv
    perm = torch.randperm(nxt + 3, generator=_gen(seed)).tolist()
    maxp = max(len(p) for p in logical) + 2
    bt = np.zeros((B, maxp), dtype=np.int32)
    rows_k, rows_v, slots = [], [], []
    for b, s in enumerate(dd["seqs"]):
        phys = [perm[x] for x in logical[b]]
        bt[b, :] = phys[-1]
        bt[b, : len(phys)] = phys
        Kf, Vf = full_view(s)
        first = nsh[b] * PAGE if (G > 1 and b % G) else 0
        pos = torch.arange(first, Kf.shape[0])
        rows_k.append(Kf[first:].reshape(len(pos), -1))
        rows_v.append(Vf[first:].reshape(len(pos), -1))
        slots.append(torch.tensor(phys)[pos // PAGE].long() * PAGE + pos % PAGE)
    assert any(bt[b, 1] != bt[b, 0] + 1 for b in range(B) if len(logical[b]) > 2), "the block table must not be the identity"
    kc = torch.zeros(nxt + 3, Hkv, PAGE, D, dtype=BF, device=dev)
    vc = torch.zeros(nxt + 3, Hkv, D, PAGE, dtype=BF, device=dev)
    ops.kv_store(torch.cat(rows_k).to(BF).to(dev), torch.cat(rows_v).to(BF).to(dev), torch.cat(slots).to(dev), kc, vc, Hkv, D)
    sp = torch.tensor([nsh[g * G] for g in range(B // G)], dtype=torch.int32, device=dev) if G > 1 else None
    return kc, vc, torch.from_numpy(bt).to(dev), sp


# ======================================================================================================================================================
# CPU part: the emulation is inside the bounds, every fault model is 4 x outside them where it was designed to show
# ======================================================================================================================================================

EMU_MAX = {}        # (kernel, output) -> largest err / (2^-6 E) of the emulation, printed by the last CPU test


def _note(key, val):
    EMU_MAX[key] = max(EMU_MAX.get(key, 0.0), float(val))


def _train_cpu(L, kernel):
    ref = run_layout(L)
    for (i, j), w in ref["needle_w"].items():
        assert w >= NEEDLE_W, f"{L['name']}: needle weight {w:.4f} at segment {i} row {j}"
    em = run_layout(L, emu=True)
    rows = inside_rows(L)
    for name in ("o", "dq", "dk", "dv"):
        _note((kernel, name), check_bound(f"emulation {name} [{L['name']}]", em[name][rows], ref[name][rows], ref["E_" + name][rows], rows.tolist()))
    _note((kernel, "lse"), check_lse(f"emulation lse [{L['name']}]", em["lse"][:, rows], ref["lse"][:, rows], rows.tolist()))
    seen = {}
    for fault in TRAIN_FAULTS:
        rows_f = designated(L, fault)
        if not rows_f:
            continue
        bad = run_layout(L, fault=fault)
        rf = torch.tensor(rows_f)
        ro = ratio(bad["o"][rf][:, L["h0"]], ref["o"][rf][:, L["h0"]], ref["E_o"][rf][:, L["h0"]]).amax(-1)       # [rows, kv groups]
        worst = ro.min()
        assert worst >= FAULT_FACTOR, (f"{L['name']}: fault '{fault}' moves o by only {float(worst):.2f} x the bound at row {rows_f[int(ro.amin(1).argmin())]} "
                                       f"(designated rows {rows_f})")
        # dq as well where the faulty row still mixes several keys (a row left with one dominant key, or with poison only, has o = V whatever the weights: its dS,
        # and so its dq, is ~0 by construction and says nothing)
        if fault in ("strict", "permissive", "other_prefix"):
            rq = ratio(bad["dq"][rf][:, L["h0"]], ref["dq"][rf][:, L["h0"]], ref["E_dq"][rf][:, L["h0"]]).amax()
            assert rq >= FAULT_FACTOR, f"{L['name']}: fault '{fault}' moves dq by only {float(rq):.2f} x the bound at its designated rows"
        if fault in ("strict", "permissive"):        # the needle KEY rows: their dv loses / gains a whole weight
            kr = torch.tensor(sorted({r + (1 if fault == "permissive" else 0) for r in rows_f}))
            rv = ratio(bad["dv"][kr], ref["dv"][kr], ref["E_dv"][kr]).amax()
            assert rv >= FAULT_FACTOR, f"{L['name']}: fault '{fault}' moves dv by only {float(rv):.2f} x the bound at the needle key rows"
        seen[fault] = float(worst)
    return seen


@pytest.mark.parametrize("idx", range(len(ATTN_CASES) + 3))
def test_cpu_training_emulation_inside_and_faults_outside(idx):
    L = plain_layouts()[idx]
    seen = _train_cpu(L, "attn_fwd/attn_bwd")
    print(f"[attn_f64 cpu] {L['name']}: smallest fault excess at designated rows (x bound) {seen}")
    want = {"before_start", "past_end"} | ({"strict", "permissive"} if L["causal"] else set())
    if idx >= len(ATTN_CASES):
        assert want <= set(seen), (want, seen)


@pytest.mark.parametrize("idx", range(len(PREFIX_CASES) + 3))
def test_cpu_shared_prefix_emulation_inside_and_faults_outside(idx):
    L = prefix_layouts()[idx]
    seen = _train_cpu(L, "shared prefix")
    print(f"[attn_f64 cpu] {L['name']}: smallest fault excess at designated rows (x bound) {seen}")
    assert {"strict", "permissive", "prefix_causal"} <= set(seen), seen
    if idx >= len(PREFIX_CASES):
        assert {"other_prefix", "past_end"} <= set(seen), seen


def _decode_faults(dd, b):
    ref = decode_ref(dd, b)
    h0 = dd["h0"]
    s = dd["seqs"][b]
    for p_ in s["needles"]:
        w = float(ref["P"][h0, 0, p_].min())
        assert w >= NEEDLE_W, f"needle weight {w:.4f} at key {p_} of n = {s['n']} ({dd['Hq']}:{dd['Hkv']})"
    seen = {}
    for fault in DECODE_FAULTS:
        bad = decode_ref(dd, b, fault=fault)
        if bad is None:
            continue
        r = ratio(bad["o"][h0], ref["o"][h0], ref["E_o"][h0]).amax(-1).min()
        assert r >= FAULT_FACTOR, f"decode fault '{fault}' moves o by only {float(r):.2f} x the bound at n = {s['n']} ({dd['Hq']}:{dd['Hkv']}), first heads of the kv groups"
        seen[fault] = float(r)
    return ref, seen


@pytest.mark.parametrize("gi", range(len(DECODE_GEOMS)))
def test_cpu_decode_emulation_inside_and_faults_outside(gi):
    dd = decode_sets()[gi]
    low = {}
    for b, n in enumerate(dd["ctx"]):
        ref, seen = _decode_faults(dd, b)
        for f, r in seen.items():
            low[f] = min(low.get(f, 1e30), r)
        o, lse = decode_emu(dd, b, wave_streams(dd["seqs"][b]["npage"]))
        _note(("attn_decode", "o"), check_bound(f"decode emulation n={n}", o.transpose(0, 1), ref["o"].transpose(0, 1), ref["E_o"].transpose(0, 1), [b]))
        _note(("attn_decode", "lse"), check_lse(f"decode emulation lse n={n}", lse, ref["lse"], [b]))
        if n == 0:
            assert bool((o == 0).all()) and bool(torch.isinf(lse).all())
    print(f"[attn_f64 cpu] decode {dd['Hq']}:{dd['Hkv']}: smallest fault excess (x bound) {low}")
    assert set(low) == set(DECODE_FAULTS) - ({"wrong_kv_head"} if dd["Hkv"] < 2 else set())


@pytest.mark.parametrize("gi", range(len(GROUP_CASES)))
def test_cpu_decode_group_emulation_inside_and_faults_outside(gi):
    dd = group_sets()[gi]
    G = dd["G"]
    for b in range(dd["B"]):
        ref, _ = _decode_faults(dd, b)
        s = dd["seqs"][b]
        for chunks in GROUP_CHUNKS:
            o, lse = decode_emu(dd, b, group_streams(s["npage"], dd["prompts"][b // G] // PAGE, chunks))
            _note(("attn_decode_group", "o"), check_bound(f"group emulation b={b} chunks={chunks}", o.transpose(0, 1), ref["o"].transpose(0, 1), ref["E_o"].transpose(0, 1), [b]))
            _note(("attn_decode_group", "lse"), check_lse(f"group emulation lse b={b}", lse, ref["lse"], [b]))


def test_cpu_every_fault_model_was_exercised_and_emulation_record():
    """Every training fault has designated rows in some input set (the per-case tests assert the 4 x there); prints the emulation's largest err / E per kernel."""
    for fault in TRAIN_FAULTS:
        assert any(designated(L, fault) for L in plain_layouts() + prefix_layouts()), fault
    for key in sorted(EMU_MAX):
        print(f"[attn_f64 cpu] emulation, {key[0]} {key[1]}: " + (f"max err = {EMU_MAX[key]:.3f} x 1e-4 max(1, |ref|)" if key[1] == "lse" else f"max err/E = {EMU_MAX[key]:.3f} x 2^-6"))


# ======================================================================================================================================================
# GPU part
# ======================================================================================================================================================

def _report(kernel, out, val):
    print(f"[attn_f64 gpu] {kernel} {out}: max err/E = {val:.3f} x 2^-6" if out != "lse" else f"[attn_f64 gpu] {kernel} lse: max err = {val:.3f} x 1e-4 max(1, |ref|)")


def _train_gpu(L, kernel):
    D, Hq, Hkv, T, sc = L["D"], L["Hq"], L["Hkv"], L["T"], L["scale"]
    qkv, do = L["qkv"].to(DEV), L["do"].to(DEV)
    q, k, v = qkv[:, : Hq * D], qkv[:, Hq * D: (Hq + Hkv) * D], qkv[:, (Hq + Hkv) * D:]
    pre = prefix_table(L) if any(p is not None for p in L["parent"]) else None
    seg = ops.Segments([s for s, _ in L["segs"]], [e for _, e in L["segs"]], DEV, prefix=pre)
    if pre is not None:
        assert (seg.n_head > 0) == ("hint off" not in L["name"]), (L["name"], seg.n_head)
    o_buf = torch.full((T, Hq * D), 7.0, dtype=BF, device=DEV)
    o, lse = ops.attn_fwd(q, k, v, seg, Hq, Hkv, D, L["causal"], sc, out=o_buf)
    dqkv = torch.full_like(qkv, 7.0)
    dq, dk, dv = dqkv[:, : Hq * D], dqkv[:, Hq * D: (Hq + Hkv) * D], dqkv[:, (Hq + Hkv) * D:]
    ops.attn_bwd(q, k, v, o, do, lse, seg, Hq, Hkv, D, L["causal"], sc, dq, dk, dv)
    torch.cuda.synchronize()
    ref = run_layout(L, dev=DEV)
    rows = inside_rows(L).to(DEV)
    names = rows.tolist()
    outside = torch.ones(T, dtype=torch.bool, device=DEV)
    outside[rows] = False
    got = {"o": o.view(T, Hq, D), "dq": dq.reshape(T, Hq, D), "dk": dk.reshape(T, Hkv, D), "dv": dv.reshape(T, Hkv, D)}
    for name in ("o", "dq", "dk", "dv"):
        _report(kernel, name, check_bound(f"{name} [{L['name']}]", got[name][rows], ref[name][rows], ref["E_" + name][rows], names))
        assert bool((got[name][outside] == 7.0).all()), f"{name} [{L['name']}]: rows outside every segment were written"
    _report(kernel, "lse", check_lse(f"lse [{L['name']}]", lse[:, rows], ref["lse"][:, rows], names))
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize("idx", range(len(ATTN_CASES) + 3))
def test_gpu_attn_fwd_bwd_against_float64(idx):
    """o, lse, dq, dk, dv of ops.attn_fwd / ops.attn_bwd on the geometries of ATTN_CASES and on segment lengths 1 .. 257 at unaligned starts with poisoned gaps;
    rows outside every segment keep what they held."""
    _train_gpu(plain_layouts()[idx], "attn_fwd/attn_bwd")


@pytest.mark.gpu
@pytest.mark.parametrize("idx", range(len(PREFIX_CASES) + 3))
def test_gpu_shared_prefix_against_float64(idx):
    """The shared-prefix form on the geometries of PREFIX_CASES (head splits 2, 4, 2, 7, 1, 4 of the dK/dV backward; the launch hint on) and on prompts of 1, 63, 64,
    65, 512 tokens with children that include length 1, prompts first (hint on) and prompts between their children (hint off).  The float64 dk / dv of a prompt hold
    every child's contribution, and so must the kernel's."""
    L = prefix_layouts()[idx]
    ref = _train_gpu(L, "shared prefix")
    # a prompt's dk without its children would be far outside: the children's share of E_dk is most of it
    for i, (s, e) in enumerate(L["segs"]):
        if any(p == i for p in L["parent"]):
            assert float(ref["E_dk"][s:e].sum()) > 0


def _decode_refs(dd):
    refs = [decode_ref(dd, b, dev=DEV) for b in range(dd["B"])]
    st = lambda key: torch.stack([r[key][:, 0] for r in refs])            # [B, Hq, D]
    return st("o"), st("E_o"), torch.stack([r["lse"][:, 0] for r in refs], 1)       # lse [Hq, B]


def _arena(dd, T):
    Hq, D = dd["Hq"], dd["D"]
    return torch.full((T, Hq * D), float("nan"), dtype=BF, device=DEV), torch.full((Hq, T), float("nan"), dtype=F32, device=DEV)


def _check_side(what, dd, arena_o, arena_l, rows, o, ref_o, ref_E, ref_lse):
    B, Hq, D = dd["B"], dd["Hq"], dd["D"]
    assert torch.equal(arena_o[rows], o), f"{what}: side rows p0 differ from the output"
    check_bound(f"{what} side p0", arena_o[rows].view(B, Hq, D), ref_o, ref_E)
    other = torch.ones(arena_o.shape[0], dtype=torch.bool, device=DEV)
    other[rows] = False
    assert bool(torch.isnan(arena_o[other]).all()) and bool(torch.isnan(arena_l[:, other]).all()), f"{what}: side rows of other steps were written"
    return check_lse(f"{what} side lse (p1)", arena_l[:, rows], ref_lse)


@pytest.mark.gpu
@pytest.mark.parametrize("gi", range(len(DECODE_GEOMS)))
def test_gpu_decode_against_float64(gi):
    """ops.attn_decode, row-major and PackedAct output, context lengths 0 .. 3185 in one batch (0 .. 100 pages against the kernel's 16 waves), cache written through
    ops.kv_store with a permuted block table, poison in every slot and page that must not be read; the side outputs (p0 rows, p1 log-sum-exp) against float64."""
    dd = decode_sets()[gi]
    Hq, Hkv, D, B = dd["Hq"], dd["Hkv"], dd["D"], dd["B"]
    kc, vc, bt, _ = paged_cache(dd, DEV, seed=gi)
    q = dd["q"].reshape(B, Hq * D).to(BF).to(DEV)
    ctx = torch.tensor(dd["ctx"], dtype=torch.int32, device=DEV)
    o = ops.attn_decode(q, kc, vc, bt, ctx, Hq, Hkv, D, dd["scale"])
    op = ops.attn_decode(q, kc, vc, bt, ctx, Hq, Hkv, D, dd["scale"], out=ops.PackedAct(B, Hq * D, DEV))
    step = torch.tensor([3], dtype=torch.int32, device=DEV)
    T = 2 + B * 8 + 5
    arena_o, arena_l = _arena(dd, T)
    o2 = ops.attn_decode(q, kc, vc, bt, ctx, Hq, Hkv, D, dd["scale"], side=ops.SideOut.make(step, 2, 8, p0=arena_o, p1=arena_l, ld1=T))
    torch.cuda.synchronize()
    ref_o, ref_E, ref_lse = _decode_refs(dd)
    _report(f"attn_decode {Hq}:{Hkv}", "o", check_bound(f"decode o {Hq}:{Hkv}", o.view(B, Hq, D), ref_o, ref_E, dd["ctx"]))
    assert torch.equal(op.unpack(), o) and torch.equal(o2, o)
    rows = 2 + torch.arange(B, device=DEV) * 8 + 3
    _report(f"attn_decode {Hq}:{Hkv}", "lse", _check_side(f"decode {Hq}:{Hkv}", dd, arena_o, arena_l, rows, o, ref_o, ref_E, ref_lse))
    z = dd["ctx"].index(0)
    assert bool((o[z] == 0).all()) and bool(torch.isinf(arena_l[:, rows[z]]).all()) and bool((arena_l[:, rows[z]] < 0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("gi", range(len(GROUP_CASES)))
def test_gpu_decode_group_against_float64(gi):
    """ops.attn_decode_group on the rollout's shared-page layout (prompts of exactly k * 32 tokens, shorter than a page, 3184 tokens; G = 8, 4, 3, 2), chunks 1, 2, 5
    and 33 (more than the shared pages): EVERY sequence and the log-sum-exp side output against float64; ops.attn_decode on the same cache as well."""
    dd = group_sets()[gi]
    Hq, Hkv, D, B, G = dd["Hq"], dd["Hkv"], dd["D"], dd["B"], dd["G"]
    kc, vc, bt, sp = paged_cache(dd, DEV, seed=10 + gi)
    q = dd["q"].reshape(B, Hq * D).to(BF).to(DEV)
    ctx = torch.tensor(dd["ctx"], dtype=torch.int32, device=DEV)
    ref_o, ref_E, ref_lse = _decode_refs(dd)
    step = torch.tensor([5], dtype=torch.int32, device=DEV)
    T = 1 + B * 6 + 7
    rows = 1 + torch.arange(B, device=DEV) * 6 + 5
    for chunks in GROUP_CHUNKS:
        arena_o, arena_l = _arena(dd, T)
        o = ops.attn_decode_group(q, kc, vc, bt, ctx, sp, G, Hq, Hkv, D, dd["scale"], chunks=chunks, side=ops.SideOut.make(step, 1, 6, p0=arena_o, p1=arena_l, ld1=T))
        torch.cuda.synchronize()
        _report(f"attn_decode_group {Hq}:{Hkv} G={G} chunks={chunks}", "o", check_bound(f"group o chunks={chunks}", o.view(B, Hq, D), ref_o, ref_E, dd["ctx"]))
        _report(f"attn_decode_group {Hq}:{Hkv} G={G} chunks={chunks}", "lse", _check_side(f"group chunks={chunks}", dd, arena_o, arena_l, rows, o, ref_o, ref_E, ref_lse))
    op = ops.attn_decode_group(q, kc, vc, bt, ctx, sp, G, Hq, Hkv, D, dd["scale"], out=ops.PackedAct(B, Hq * D, DEV))
    assert torch.equal(op.unpack(), ops.attn_decode_group(q, kc, vc, bt, ctx, sp, G, Hq, Hkv, D, dd["scale"]))
    o_seq = ops.attn_decode(q, kc, vc, bt, ctx, Hq, Hkv, D, dd["scale"], seqs_per_group=G)
    _report(f"attn_decode on the shared-page layout {Hq}:{Hkv}", "o", check_bound("per-sequence decode on the shared-page layout", o_seq.view(B, Hq, D), ref_o, ref_E, dd["ctx"]))


CHUNK_CASES = [  # Hq, Hkv, prompts Bp, prompt length S, G, completion length C, blk_log2, chunk boundaries (logical rows; the last is C)
    (4, 2, 2, 70, 3, 96, 4, [16, 17, 48, 96]),
    (16, 2, 1, 129, 4, 160, 5, [32, 37, 96, 97, 160]),
    (28, 4, 2, 33, 2, 64, 4, [16, 64]),
]


@pytest.mark.gpu
@pytest.mark.parametrize("Hq,Hkv,Bp,S,G,C,blk,cuts", CHUNK_CASES)
def test_gpu_attn_fwd_chunk_bit_equal_and_against_float64(Hq, Hkv, Bp, S, G, C, blk, cuts):
    """iadr1_attn_fwd_chunk on a shared-prefix layout whose completion rows are time-blocked (blk_log2 4 and 5, blk_stride = nseq * 2^blk_log2), processed in chunks
    with seg_end growing as rows are 'written' (the rows not yet written hold poison); q_first values that are no multiple of 64 (16, 17, 37, 97) and q_count = 1.
    Every chunk's rows are bit-equal to ONE ops.attn_fwd over the finished sequences (contiguous layout), gathered through the row map, and within 2^-6 E of
    float64; rows outside the chunk keep what they held."""
    D, N, BLK = 128, Bp * G, 1 << blk
    assert C % BLK == 0
    T0 = Bp * S
    segs = [(b * S, (b + 1) * S) for b in range(Bp)] + [(T0 + s_ * C, T0 + (s_ + 1) * C) for s_ in range(N)]
    L = make_layout(D, Hq, Hkv, True, segs, parent=[None] * Bp + [s_ // G for s_ in range(N)], seed=70 + blk, name="chunked forward, finished sequences")
    T, sc = L["T"], L["scale"]
    qkv = L["qkv"].to(DEV)
    W = qkv.shape[1]
    q, k, v = qkv[:, : Hq * D], qkv[:, Hq * D: (Hq + Hkv) * D], qkv[:, (Hq + Hkv) * D:]
    seg = ops.Segments([s for s, _ in segs], [e for _, e in segs], DEV, prefix=prefix_table(L))
    o_full, lse_full = ops.attn_fwd(q, k, v, seg, Hq, Hkv, D, True, sc)
    ref = run_layout(L, dev=DEV, backward=False)
    # the time-blocked layout: logical row j of sequence s_ at T0 + (j >> blk) * N * BLK + s_ * BLK + (j & (BLK - 1))
    j = torch.arange(C, device=DEV)
    rmap = torch.stack([T0 + (j >> blk) * (N * BLK) + s_ * BLK + (j & (BLK - 1)) for s_ in range(N)])         # [N, C] flat rows of the blocked layout
    cont = torch.stack([T0 + s_ * C + j for s_ in range(N)])                                                    # ... and of the contiguous one
    Tb = T0 + N * C + 5
    anchor_q = qkv[cont[:, 0]][:, : Hq * D].reshape(N, Hq, D)[:, L["h0"].to(DEV)]                                 # poison of a sequence's unwritten rows: K = 4 q of its first row
    qb = torch.zeros(Tb, W, dtype=BF, device=DEV)
    qb[:T0] = qkv[:T0]
    qb[rmap.reshape(-1)] = qkv[cont.reshape(-1)]
    written = qb.clone()
    poison = qb.clone()
    poison[rmap.reshape(-1), Hq * D: (Hq + Hkv) * D] = (4.0 * anchor_q.float()).to(BF).reshape(N, 1, Hkv * D).expand(N, C, Hkv * D).reshape(N * C, Hkv * D)
    poison[rmap.reshape(-1), (Hq + Hkv) * D:] = 100.0
    seg_start = torch.tensor([T0 + s_ * BLK for s_ in range(N)], dtype=torch.int32, device=DEV)
    seg_prefix = torch.tensor([[(s_ // G) * S, S, 0, 0] for s_ in range(N)], dtype=torch.int32, device=DEV)
    o_b = torch.full((Tb, Hq * D), 7.0, dtype=BF, device=DEV)
    lse_b = torch.full((Hq, Tb), 7.0, dtype=F32, device=DEV)
    worst, c0 = 0.0, 0
    for c1 in cuts:
        cur = poison.clone()                                          # rows [0, c1) written, the rest poison
        cur[rmap[:, :c1].reshape(-1)] = written[rmap[:, :c1].reshape(-1)]
        seg_end = (seg_start + c1).to(torch.int32)
        view = torch.tensor([[c0, c1 - c0, blk, N * BLK]] * N, dtype=torch.int32, device=DEV)
        before_o, before_l = o_b.clone(), lse_b.clone()
        ops.hip.call("attn_fwd_chunk", cur[:, : Hq * D], cur[:, Hq * D: (Hq + Hkv) * D], cur[:, (Hq + Hkv) * D:], o_b, lse_b, seg_start, seg_end, seg_prefix, view, N, c1 - c0,
                     Tb, Hq, Hkv, D, W, W, W, Hq * D, sc)
        torch.cuda.synchronize()
        rb, rc = rmap[:, c0:c1].reshape(-1), cont[:, c0:c1].reshape(-1)
        assert torch.equal(o_b[rb], o_full[rc]), f"chunk [{c0}, {c1}): rows differ from attn_fwd over the finished sequences"
        assert torch.equal(lse_b[:, rb], lse_full[:, rc]), f"chunk [{c0}, {c1}): log-sum-exp differs from attn_fwd over the finished sequences"
        worst = max(worst, check_bound(f"chunk [{c0}, {c1}) o", o_b[rb].view(-1, Hq, D), ref["o"][rc], ref["E_o"][rc], rc.tolist()))
        check_lse(f"chunk [{c0}, {c1}) lse", lse_b[:, rb], ref["lse"][:, rc], rc.tolist())
        keep = torch.ones(Tb, dtype=torch.bool, device=DEV)
        keep[rb] = False
        assert torch.equal(o_b[keep], before_o[keep]) and torch.equal(lse_b[:, keep], before_l[:, keep]), f"chunk [{c0}, {c1}): rows outside the chunk were written"
        c0 = c1
    assert c0 == C
    _report("attn_fwd_chunk", "o", worst)
