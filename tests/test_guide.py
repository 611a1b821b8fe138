"""iadr1_amd.guide, the host side of regex-guided decoding (trl's vllm_guided_decoding_regex): pattern -> byte DFA -> the sampler's allow / trans tables.  The oracle
of the dialect is Python's `re` in bytes mode, re.fullmatch(pattern.encode(), data), with no caveats; the token level is checked against the byte DFA, which is
checked against `re`.  Nothing here needs a GPU."""
import functools
import importlib.util
import os
import random
import re
import zlib

import numpy as np
import pytest

import iadr1_amd  # noqa: F401
from iadr1_amd import guide

RECIPE = r"<think>[\s\S]*?</think><location>[^<]+</location><type>[a-z ]{1,20}</type><answer>(Yes|No)</answer>"
# together: literals, \n \t \r \\ and escaped punctuation, \xNN, \d \w \s \D \W \S, classes with ranges / negation / escapes inside, '.', capturing and (?:) groups,
# alternation (nested, with an empty branch), * + ? {m} {m,} {m,n} {,n} and the lazy form of each
PATTERNS = [
    RECIPE,
    r"a{2,4}b+?(c|d(e|f)*)?x*",
    r"[^a-c\n]+x\.\d\W",
    r"(?:ab|a)*\x41{2}.?",
    r"\w+@\w+\.(com|org|net)",
    r"\s*-?\d{1,3}(,\d{3})*(\.\d+)?\s*",
    r"[\]\-a\\]+\t\r?\n",
    r"\D{2,}\S\s??[^\w]",
    r"(a|b|)(c(d|e(f|g))|h)*z{,3}",
    r"[0-9a-fA-F]{2}(:[0-9a-fA-F]{2}){2,5}",
    r".*\\n.+?",
    r"[^\x00-\x7f]+!*?",
    r"x{3}[yY]{2,}?[z0-9]{1,2}?w{2}?",
    r"[\d\s]+[^\D5]*\(\[\{\|\}\]\)",
]


@functools.lru_cache(maxsize=None)
def dfa_of(pattern):
    return guide.compile_regex(pattern)


def to_accept(dfa):
    """Distance (in bytes) of every state to an accepting one."""
    dist = np.where(dfa.accept, 0, 10 ** 9)
    while True:
        nxt = np.where(dfa.trans >= 0, dist[np.maximum(dfa.trans, 0)], 10 ** 9).min(1) + 1
        new = np.minimum(dist, nxt)
        if (new == dist).all():
            return dist
        dist = new


def random_walk(dfa, dist, rng):
    """A string the DFA accepts by construction: random allowed bytes, then (or with probability 1/4 at every step) downhill towards acceptance."""
    s, out = 0, bytearray()
    while True:
        ok = np.flatnonzero(dfa.trans[s] >= 0)
        if dfa.accept[s] and (rng.random() < 0.12 or len(out) > 60 or not len(ok)):
            return bytes(out)
        if len(out) > 40 or rng.random() < 0.25:
            down = [b for b in ok if dist[dfa.trans[s, b]] < dist[s]]
            ok = down or ok
        b = int(rng.choice(list(ok)))
        out.append(b)
        s = int(dfa.trans[s, b])


def edit(data, alphabet, rng):
    data = bytearray(data)
    kind = rng.randrange(3)
    pos = rng.randrange(len(data) + 1)
    if kind == 0 or not data:
        data.insert(pos, rng.choice(alphabet))
    elif kind == 1:
        del data[min(pos, len(data) - 1)]
    else:
        data[min(pos, len(data) - 1)] = rng.choice(alphabet)
    return bytes(data)


@pytest.mark.parametrize("pattern", PATTERNS)
def test_dfa_agrees_with_re_in_bytes_mode(pattern):
    """dfa.accepts(b) == bool(re.fullmatch(pattern.encode(), b)) on strings drawn three ways: random walks through the DFA, single-byte edits of those, random bytes
    (values >= 0x80 and \\n among them).  At least 100 distinct accepted and 100 distinct rejected strings per pattern, asserted on the test's own inputs."""
    dfa, rx, rng = dfa_of(pattern), re.compile(pattern.encode()), random.Random(zlib.crc32(pattern.encode()))
    assert dfa.trans.shape == (dfa.n, 256) and dfa.accept.shape == (dfa.n,)
    dist = to_accept(dfa)
    assert (dist < 10 ** 9).all(), "a state that cannot reach acceptance survived the trim"
    alphabet = bytes(sorted(set(pattern.encode()) | set(b"\n\t\r .,:5aZ_\x00\x7f\x80\xa9\xc3\xff")))
    walks = [random_walk(dfa, dist, rng) for _ in range(400)]
    strings = set(walks)
    for w in walks:
        strings.add(edit(w, alphabet, rng))
        strings.add(edit(edit(w, alphabet, rng), alphabet, rng))
    for _ in range(400):
        strings.add(bytes(rng.choice(alphabet) for _ in range(rng.randrange(0, 12))))
    yes = no = 0
    for b in sorted(strings):
        want = bool(rx.fullmatch(b))
        assert dfa.accepts(b) == want, (pattern, b, want)
        yes, no = yes + want, no + (not want)
    assert all(rx.fullmatch(w) for w in walks)
    assert yes >= 100 and no >= 100, (pattern, yes, no)


def test_minimisation_and_start_state():
    """Moore refinement: equivalent spellings of one language give DFAs of the same size, the known minimal sizes come out, the start state is 0."""
    assert dfa_of(r"(a|b)*abb").n == 4                   # the textbook example
    assert dfa_of(r"a*").n == 1 and dfa_of(r"").n == 1 and dfa_of(r"(Yes|No)").n == 5      # Y-e-s / N-o share the accepting state
    assert dfa_of(r"(?:ab|a)*").n == guide.compile_regex(r"(a|ab)*?").n == guide.compile_regex(r"(ab?)*").n
    assert dfa_of(r"x{2,3}").n == guide.compile_regex(r"xxx?").n == 4
    d = dfa_of(r"[^\s\S]")                               # the empty language: one state, nothing accepted
    assert d.n == 1 and not d.accepts(b"") and not d.accepts(b"a")


REFUSED = [
    (r"^abc", "anchor"), (r"abc$", "anchor"), (r"\bword", "anchor"), (r"a\Z", "anchor"), (r"(a)\1", "backreference"), (r"(?P<n>a)(?P=n)", "named group"),
    (r"(?P=n)", "backreference"), (r"a(?=b)", "look-around"), (r"a(?!b)", "look-around"), (r"(?<=a)b", "look-around"), (r"(?<!a)b", "look-around"),
    (r"(?i)abc", "flags"), (r"(?P<name>a)", "named group"), ("café", "non-ASCII"), (r"a**", "multiple repeat"), (r"a*+", "possessive"), (r"a{3,2}", "min > max"),
    (r"[z-a]", "reversed range"), (r"[a-\d]", "class escape"), (r"(ab", "unbalanced"), (r"ab)", "unbalanced"), (r"*a", "nothing to repeat"), (r"a{2", "'{'"),
    (r"\p", "escape"), (r"[abc", "unterminated"), ("ab\\", "trailing backslash"), (r"(?#c)a", "comment"), (r"(?>a)", "atomic"), (r"a{2000}", "repeat count"),
    (r"\x4", "hex"),
]


@pytest.mark.parametrize("pattern,word", REFUSED)
def test_unsupported_constructs_are_refused_by_name(pattern, word):
    with pytest.raises(ValueError, match=re.escape(word)) as ei:
        guide.compile_regex(pattern)
    assert "position" in str(ei.value)


# ---- token_bytes: one synthetic tokenizer per kind ---------------------------------------------------------------------------------------------------------

def test_token_bytes_byte_level():
    """GPT-2's unicode-to-byte map, expectations written out by hand: U+0120 is the space, U+010A the newline, U+0122 the lone byte 0x80, 'Ã©' the two bytes of e-acute."""
    from tokenizers import Tokenizer, decoders, models, pre_tokenizers
    from transformers import PreTrainedTokenizerFast
    vocab = {"a": 0, "Ġthe": 1, "Ċ": 2, "Ģ": 3, "Ã©": 4, "</": 5, "ĠĠ": 6, "!": 7}
    tok = Tokenizer(models.BPE(vocab=vocab, merges=[]))
    tok.pre_tokenizer = pre_tokenizers.ByteLevel(add_prefix_space=False)
    tok.decoder = decoders.ByteLevel()
    fast = PreTrainedTokenizerFast(tokenizer_object=tok, eos_token="<|im_end|>", pad_token="<|endoftext|>")
    assert len(fast) == 10
    got = guide.token_bytes(fast, 16)
    assert got == [b"a", b" the", b"\n", b"\x80", b"\xc3\xa9", b"</", b"  ", b"!", None, None] + [None] * 6
    only_pre = Tokenizer(models.BPE(vocab=vocab, merges=[]))
    only_pre.pre_tokenizer = pre_tokenizers.ByteLevel(add_prefix_space=False)
    assert guide.token_bytes(only_pre, 8) == got[:8]


def test_token_bytes_sentencepiece_style():
    """U+2581 is a space and <0xNN> that byte: with a Metaspace decoder, and with a LLaMA-style decoder chain that is recognised by its vocabulary."""
    from tokenizers import Tokenizer, decoders, models
    vocab = {"<unk>": 0, "<s>": 1, "</s>": 2, "<0x0A>": 3, "<0xE2>": 4, "▁the": 5, "▁": 6, "a": 7, "é": 8, "▁▁": 9, "<0x>": 10}
    want = [None, None, None, b"\n", b"\xe2", b" the", b" ", b"a", b"\xc3\xa9", b"  ", b"<0x>", None]
    for dec in (decoders.Metaspace(), decoders.Sequence([decoders.Replace("▁", " "), decoders.ByteFallback(), decoders.Fuse()])):
        tok = Tokenizer(models.BPE(vocab=vocab, merges=[], unk_token="<unk>", byte_fallback=True))
        tok.decoder = dec
        tok.add_special_tokens(["<unk>", "<s>", "</s>"])
        assert guide.token_bytes(tok, 12) == want


def test_token_bytes_word_level_and_refusal():
    """No decoder: the token string in UTF-8; specials and the ids up to the padded vocabulary size are None; a tokenizer with another decoder is refused by name."""
    from tokenizers import Tokenizer, decoders, models
    from transformers import PreTrainedTokenizerFast
    words = ["<pad>", "<eos>", "a", "\n", "é", "<", "think"]
    tok = Tokenizer(models.WordLevel({w: i for i, w in enumerate(words)}, unk_token="<pad>"))
    fast = PreTrainedTokenizerFast(tokenizer_object=tok, eos_token="<eos>", pad_token="<pad>")
    assert guide.token_bytes(fast, 9) == [None, None, b"a", b"\n", b"\xc3\xa9", b"<", b"think", None, None]
    assert guide.token_bytes(fast, 4) == [None, None, b"a", b"\n"]       # a model vocabulary smaller than the tokenizer's: the ids beyond it are dropped
    piece = Tokenizer(models.WordPiece({"[UNK]": 0, "a": 1, "##b": 2}, unk_token="[UNK]"))
    piece.decoder = decoders.WordPiece()
    with pytest.raises(ValueError, match="WordPiece"):
        guide.token_bytes(piece, 3)
    with pytest.raises(ValueError, match="fast tokenizer"):
        guide.token_bytes(object(), 3)


# ---- TokenGuide ----------------------------------------------------------------------------------------------------------------------------------------------

TOY_PATTERN = r"<think>[\s\S]*?</think>(yes|no)"
# every byte the pattern needs as a single token, multi-byte tokens that straddle the literals' boundaries, a lone UTF-8 continuation byte, a two-byte character,
# a special (None) in the middle, the EOS at id 3 and one padding id at the end
TOY = [b"<", b">", b"/", None, b"t", b"h", b"i", b"n", b"k", b"y", b"e", b"s", b"o", b"</", b"k>", b"think", b"<think>", b"nk></", b"\x80", b"\xc3\xa9", None,
       b"a", b" ", b"\n", b">y", b"hink>no", b"</think>yes", b"ye", b"es", None]
TOY_EOS = 3


@functools.lru_cache(maxsize=None)
def toy_guide():
    return guide.TokenGuide.build(dfa_of(TOY_PATTERN), TOY, TOY_EOS, len(TOY))


def test_guide_tables_are_consistent():
    g, V = toy_guide(), len(TOY)
    assert g.trans.dtype == np.int16 and g.trans.shape == (g.S, V) and g.allow.dtype == np.uint32 and g.allow.shape == (g.S, (V + 31) // 32)
    assert g.start == 0 and g.V == V and g.eos_id == TOY_EOS and 1 <= g.S <= 32767 and g.nbytes == g.trans.nbytes + g.allow.nbytes
    bits = (g.allow[:, np.arange(V) >> 5] >> (np.arange(V) & 31).astype(np.uint32)) & 1
    assert np.array_equal(bits.astype(bool), g.trans >= 0), "allow is the bitmap of trans >= 0"
    assert (g.allow[:, -1] >> np.uint32(V & 31) == 0).all(), "bits beyond V are clear"
    assert (g.trans < g.S).all() and (g.trans >= -1).all()
    eos = g.trans[:, TOY_EOS]
    assert np.array_equal(eos >= 0, g.accepting) and g.accepting.any() and (eos[g.accepting] == np.flatnonzero(g.accepting)).all(), "EOS only in accepting states, and it loops"
    assert np.array_equal(g.accepting, dfa_of(TOY_PATTERN).accept[g.byte_state])
    assert (g.trans >= 0).any(1).all(), "every state allows a token"
    for none_id in (i for i, b in enumerate(TOY) if b is None and i != TOY_EOS):
        assert (g.trans[:, none_id] == -1).all()
    reach, todo = {0}, [0]          # every state is reachable from the start by tokens
    while todo:
        for u in set(g.trans[todo.pop()].tolist()) - {-1} - reach:
            reach.add(u)
            todo.append(u)
    assert reach == set(range(g.S))


def test_guide_allows_exactly_the_live_token_sequences():
    """2000 random token sequences (a walk along allowed tokens that strays with probability 0.12 per token, an EOS or two behind a third of them): the guide
    allows the sequence exactly when no token is unemittable, the concatenated bytes keep the byte DFA alive and an EOS stands only where they match."""
    g, dfa, rng = toy_guide(), dfa_of(TOY_PATTERN), random.Random(7)
    V = len(TOY)
    yes = no = ended = 0
    for _ in range(2000):
        ids, s = [], 0
        for _ in range(rng.randrange(1, 14)):
            ok = [t for t in np.flatnonzero(g.trans[s] >= 0).tolist() if t != TOY_EOS] if s >= 0 else []
            t = rng.choice(ok) if ok and rng.random() > 0.12 else rng.choice([t for t in range(V) if t != TOY_EOS])
            ids.append(t)
            s = int(g.trans[s, t]) if s >= 0 else -1
        n_eos = rng.choice([0, 0, 1, 2])
        data = b"".join(TOY[t] or b"" for t in ids)
        want = all(TOY[t] is not None for t in ids) and dfa.live(data) and (n_eos == 0 or dfa.accepts(data))
        got = g.walk(ids + [TOY_EOS] * n_eos)
        assert (got >= 0) == want, (ids, n_eos, data, got)
        if want:
            assert g.byte_state[got] == dfa.walk(data)
            ended += n_eos > 0
        yes, no = yes + want, no + (not want)
    assert yes >= 300 and no >= 300 and ended >= 20, (yes, no, ended)


def test_guide_prunes_what_the_vocabulary_cannot_finish():
    """(ab|cd) without a token for 'd': 'c' keeps the byte DFA alive but no token sequence behind it reaches a match, so the guide does not allow it; a pattern
    the vocabulary cannot complete at all is refused at build, and so are tables beyond the limits, with S, V and the byte count in the message."""
    vocab = [b"a", b"b", b"c", None, b"ab"]
    d = guide.compile_regex(r"(ab|cd)")
    assert d.live(b"c")
    g = guide.TokenGuide.build(d, vocab, 3, 5)
    assert g.walk([2]) == -1 and g.walk([0, 1, 3]) >= 0 and g.walk([4, 3, 3]) >= 0 and g.walk([0, 3]) == -1
    assert sorted(np.flatnonzero(g.trans[0] >= 0).tolist()) == [0, 4]
    with pytest.raises(ValueError, match="cannot be completed with this vocabulary"):
        guide.TokenGuide.build(guide.compile_regex(r"cd+"), vocab, 3, 5)
    with pytest.raises(ValueError, match=r"S = \d+ states.*V = 151936 tokens = \d+ bytes"):
        guide.TokenGuide.build(guide.ByteDFA(np.zeros((4000, 256), dtype=np.int32), np.ones(4000, dtype=bool)), [b"a"] * 151936, 3, 151936)       # 1.29 GB
    with pytest.raises(ValueError, match=r"S = 40000 states \(limit 32767\)"):
        guide.TokenGuide.build(guide.ByteDFA(np.zeros((40000, 256), dtype=np.int32), np.ones(40000, dtype=bool)), vocab, 3, 5)
    with pytest.raises(ValueError, match="eos_id"):
        guide.TokenGuide.build(d, vocab, 5, 5)


# ---- configuration ---------------------------------------------------------------------------------------------------------------------------------------------

def _grpo_ad():
    spec = importlib.util.spec_from_file_location("grpo_ad_flags_guide", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "train", "stage_rl", "grpo_ad.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_config_flag_and_yaml_set_the_pattern(tmp_path):
    from iadr1_amd.sc_grpo import GRPOArgs
    from iadr1_amd.trainer import GRPOConfig
    assert GRPOConfig().vllm_guided_decoding_regex is None and GRPOArgs().guide is None
    mod = _grpo_ad()
    base = ["--model_name_or_path", "/m", "--output_dir", "o", "--dataset_name", "d.json"]
    assert mod.build_parser().parse_args(base).vllm_guided_decoding_regex is None
    a = mod.build_parser().parse_args(base + ["--vllm_guided_decoding_regex", r"<a>(x|y){1,3}</a>"])
    assert a.vllm_guided_decoding_regex == r"<a>(x|y){1,3}</a>"
    f = tmp_path / "c.yaml"
    f.write_text("model_name_or_path: /m\noutput_dir: o\ndataset_name: d.json\nvllm_guided_decoding_regex: '<answer>(Yes|No)</answer>'\n")
    a = mod.parse_args_and_config(mod.build_parser(), ["--config", str(f)])
    assert a.vllm_guided_decoding_regex == "<answer>(Yes|No)</answer>"
    cfg = GRPOConfig(**{k: getattr(a, k) for k in GRPOConfig.__dataclass_fields__ if hasattr(a, k) and getattr(a, k) is not None and k not in ("report_to", "bf16", "push_to_hub")})
    assert cfg.vllm_guided_decoding_regex == "<answer>(Yes|No)</answer>"


def test_a_bad_pattern_fails_when_the_trainer_is_built():
    """Before any weight is loaded: the model path does not exist."""
    from iadr1_amd.sc_grpo import GRPOArgs, SCGRPOEngine
    from iadr1_amd.trainer import GRPOConfig, SCGRPOTrainer
    with pytest.raises(ValueError, match=r"vllm_guided_decoding_regex.*anchor"):
        SCGRPOTrainer("/nowhere/qwen2.5-vl-3b", [], GRPOConfig(vllm_guided_decoding_regex=r"^<answer>"))
    with pytest.raises(ValueError, match=r"vllm_guided_decoding_regex.*look-around"):
        SCGRPOTrainer("/nowhere/qwen2.5-vl-3b", [], GRPOConfig(vllm_guided_decoding_regex=r"a(?=b)"))
    with pytest.raises(ValueError, match="suppress_eos"):
        SCGRPOEngine(None, None, None, GRPOArgs(guide=toy_guide(), suppress_eos=True))
