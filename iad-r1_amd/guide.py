"""Regex-guided decoding, host side: trl's GRPOConfig(vllm_guided_decoding_regex) (REF trl/trl/trainer/grpo_config.py:294, handed to vLLM at grpo_trainer.py:629,945).

  compile_regex(pattern)                      a byte-level DFA of the pattern (our own parser: Thompson NFA -> subset construction -> trim -> Moore minimisation)
  token_bytes(tokenizer, vocab_size)          the byte string every token id stands for, None for ids that may never be emitted
  TokenGuide.build(dfa, bytes, eos, V)        the two tables the sampler reads on the device (iadr1_sample_guided): allow [S, ceil(V / 32)] and trans [S, V]

Semantics: full match over the completion's UTF-8 bytes, exactly Python's `re` in bytes mode -- re.fullmatch(pattern.encode(), text.encode()) is the oracle.
`.` is any byte but 0x0A; \\d \\w \\s are ASCII; negated classes and \\D \\W \\S match the bytes >= 0x80.  Lazy quantifiers denote the language of the greedy ones.
numpy only: nothing here touches the GPU."""
from __future__ import annotations

import json
import time

import numpy as np

ALL = (1 << 256) - 1
_DIGIT = sum(1 << c for c in range(0x30, 0x3A))
_WORD = _DIGIT | sum(1 << c for c in range(0x41, 0x5B)) | sum(1 << c for c in range(0x61, 0x7B)) | (1 << 0x5F)
_SPACE = sum(1 << c for c in b" \t\n\r\f\v")
_CLASS = {"d": _DIGIT, "w": _WORD, "s": _SPACE, "D": ALL ^ _DIGIT, "W": ALL ^ _WORD, "S": ALL ^ _SPACE}
_CTRL = {"n": 0x0A, "t": 0x09, "r": 0x0D, "f": 0x0C, "v": 0x0B}
_PUNCT = set("!\"#$%&'()*+,-./:;<=>?@[\\]^_`{|}~ ")
MAX_REPEAT = 1000          # {m,n} is expanded into copies: a bound far above anything a completion format needs
MAX_STATES = 32767         # trans holds int16
MAX_TABLE_BYTES = 1 << 30


def _popcount(x: int) -> int:
    return bin(x).count("1")


# ---- parser: pattern -> tree ---------------------------------------------------------------------------------------------------------------------------------
# tree nodes: ("set", mask) one byte out of a 256-bit mask | ("cat", [nodes]) | ("alt", [nodes]) | ("rep", node, lo, hi or None)

class _Parser:
    def __init__(self, pattern: str):
        if not isinstance(pattern, str):
            raise ValueError(f"the pattern must be a str, got {type(pattern).__name__}")
        for i, ch in enumerate(pattern):
            if ord(ch) > 127:
                raise ValueError(f"non-ASCII character {ch!r} at position {i}: the pattern must be ASCII (write other bytes as \\xNN)")
        self.p, self.i = pattern, 0

    def err(self, what, pos=None):
        return ValueError(f"unsupported in a guided-decoding regex: {what} at position {self.i if pos is None else pos} of {self.p!r}")

    def peek(self, n=1):
        return self.p[self.i: self.i + n]

    def parse(self):
        node = self.alt()
        if self.i < len(self.p):       # only an unmatched ')' stops alt() early
            raise self.err("unbalanced ')'")
        return node

    def alt(self):
        branches = [self.cat()]
        while self.peek() == "|":
            self.i += 1
            branches.append(self.cat())
        return branches[0] if len(branches) == 1 else ("alt", branches)

    def cat(self):
        items = []
        while self.i < len(self.p) and self.peek() not in ("|", ")"):
            items.append(self.quantified())
        return ("cat", items)

    def quantified(self):
        start = self.i
        ch = self.peek()
        if ch in ("*", "+", "?"):
            raise self.err(f"quantifier {ch!r} with nothing to repeat")
        if ch == "{":
            raise self.err("unescaped '{' with nothing to repeat (write \\{ for the character)")
        atom = self.atom()
        q = self.quantifier()
        if q is None:
            return atom
        nxt = self.peek()
        if nxt == "?":                  # lazy: the same language
            self.i += 1
            nxt = self.peek()
        elif nxt == "+":
            raise self.err("possessive quantifier")
        if nxt in ("*", "+", "?") or (nxt == "{" and self._braces() is not None):
            raise self.err("multiple repeat (a quantifier on a quantifier)")
        lo, hi = q
        if hi is not None and hi < lo:
            raise self.err(f"repeat bounds {{{lo},{hi}}} with min > max", start)
        if lo > MAX_REPEAT or (hi or 0) > MAX_REPEAT:
            raise self.err(f"repeat count above {MAX_REPEAT}", start)
        return ("rep", atom, lo, hi)

    def _braces(self):
        """(lo, hi, length) of a {m} {m,} {,n} {m,n} at the cursor, None when the text there is not one."""
        j = self.i + 1
        lo = ""
        while j < len(self.p) and self.p[j].isdigit():
            lo += self.p[j]
            j += 1
        hi = lo
        comma = j < len(self.p) and self.p[j] == ","
        if comma:
            j += 1
            hi = ""
            while j < len(self.p) and self.p[j].isdigit():
                hi += self.p[j]
                j += 1
        if j >= len(self.p) or self.p[j] != "}" or (not lo and not comma):
            return None
        return (int(lo) if lo else 0, (int(hi) if hi else None) if comma else int(lo), j + 1 - self.i)

    def quantifier(self):
        ch = self.peek()
        if ch == "*":
            self.i += 1
            return 0, None
        if ch == "+":
            self.i += 1
            return 1, None
        if ch == "?":
            self.i += 1
            return 0, 1
        if ch == "{":
            b = self._braces()
            if b is None:
                raise self.err("unescaped '{' that is not a {m}, {m,} or {m,n} quantifier (write \\{ for the character)")
            self.i += b[2]
            return b[0], b[1]
        return None

    def atom(self):
        ch = self.peek()
        if ch == "(":
            return self.group()
        if ch == "[":
            return ("set", self.char_class())
        if ch == ".":
            self.i += 1
            return ("set", ALL ^ (1 << 0x0A))
        if ch in ("^", "$"):
            raise self.err(f"anchor {ch!r} (the match is a full match already)")
        if ch == "\\":
            return ("set", self.escape(in_class=False))
        self.i += 1
        return ("set", 1 << ord(ch))

    def group(self):
        start = self.i
        self.i += 1
        if self.peek() == "?":
            two, three = self.peek(2), self.peek(3)
            if two == "?:":
                self.i += 2
            elif two in ("?=", "?!") or three in ("?<=", "?<!"):
                raise self.err(f"look-around ({three if three in ('?<=', '?<!') else two}...)", start)
            elif three == "?P=":
                raise self.err("backreference (?P=name)", start)
            elif three == "?P<" or two == "?<":
                raise self.err("named group (?P<name>...)", start)
            elif two == "?#":
                raise self.err("comment group (?#...)", start)
            elif two == "?>":
                raise self.err("atomic group (?>...)", start)
            elif two == "?(":
                raise self.err("conditional group (?(...)...)", start)
            else:
                raise self.err("inline flags (?...)", start)
        node = self.alt()
        if self.peek() != ")":
            raise self.err("unbalanced '(' (no closing parenthesis)", start)
        self.i += 1
        return node

    def escape(self, in_class):
        """The byte set of the escape at the cursor."""
        start = self.i
        self.i += 1
        if self.i >= len(self.p):
            raise self.err("a trailing backslash", start)
        ch = self.p[self.i]
        self.i += 1
        if ch in _CLASS:
            return _CLASS[ch]
        if ch in _CTRL:
            return 1 << _CTRL[ch]
        if ch == "x":
            hx = self.p[self.i: self.i + 2]
            if len(hx) != 2 or any(c not in "0123456789abcdefABCDEF" for c in hx):
                raise self.err("\\x without two hex digits", start)
            self.i += 2
            return 1 << int(hx, 16)
        if ch in _PUNCT:
            return 1 << ord(ch)
        if ch.isdigit():
            raise self.err(f"backreference or octal escape \\{ch}", start)
        if ch in "AZbB" and not in_class:
            raise self.err(f"anchor \\{ch}", start)
        raise self.err(f"escape \\{ch}", start)

    def char_class(self):
        start = self.i
        self.i += 1
        negate = self.peek() == "^"
        if negate:
            self.i += 1
        mask, first = 0, True
        while True:
            if self.i >= len(self.p):
                raise self.err("unterminated character class '['", start)
            ch = self.peek()
            if ch == "]" and not first:
                self.i += 1
                break
            first = False
            lo, lo_pos = self._class_item()
            if self.peek() == "-" and self.peek(2) not in ("-]", "-"):      # a range, unless the '-' is the last character of the class
                if _popcount(lo) != 1:
                    raise self.err("a range whose end point is a class escape", lo_pos)
                self.i += 1
                hi, hi_pos = self._class_item()
                if _popcount(hi) != 1:
                    raise self.err("a range whose end point is a class escape", hi_pos)
                a, b = lo.bit_length() - 1, hi.bit_length() - 1
                if b < a:
                    raise self.err(f"a reversed range \\x{a:02x}-\\x{b:02x}", lo_pos)
                mask |= ((1 << (b + 1)) - 1) ^ ((1 << a) - 1)
            else:
                mask |= lo
        return (ALL ^ mask) if negate else mask

    def _class_item(self):
        pos = self.i
        if self.peek() == "\\":
            return self.escape(in_class=True), pos
        ch = self.peek()
        self.i += 1
        return 1 << ord(ch), pos


# ---- Thompson NFA ------------------------------------------------------------------------------------------------------------------------------------------------

class _NFA:
    def __init__(self):
        self.eps, self.edge = [], []      # per state: epsilon targets; (mask, target) or None

    def new(self):
        self.eps.append([])
        self.edge.append(None)
        return len(self.eps) - 1

    def build(self, node):
        """-> (entry, exit) of a fragment for the tree node; every call makes fresh states, so a repeat builds its copies by calling again."""
        kind = node[0]
        if kind == "set":
            a, b = self.new(), self.new()
            self.edge[a] = (node[1], b)
            return a, b
        if kind == "cat":
            a = b = self.new()
            for sub in node[1]:
                s, e = self.build(sub)
                self.eps[b].append(s)
                b = e
            return a, b
        if kind == "alt":
            a, b = self.new(), self.new()
            for sub in node[1]:
                s, e = self.build(sub)
                self.eps[a].append(s)
                self.eps[e].append(b)
            return a, b
        _, sub, lo, hi = node
        a = b = self.new()
        for _ in range(lo):
            s, e = self.build(sub)
            self.eps[b].append(s)
            b = e
        if hi is None:                    # sub*
            s, e = self.build(sub)
            hub = self.new()
            self.eps[b].append(hub)
            self.eps[hub].append(s)
            self.eps[e].append(hub)
            return a, hub
        end = self.new()
        for _ in range(hi - lo):          # (sub(sub(...)?)?)?
            self.eps[b].append(end)
            s, e = self.build(sub)
            self.eps[b].append(s)
            b = e
        self.eps[b].append(end)
        return a, end


class ByteDFA:
    """trans [n, 256] int32 (-1: no such transition), accept [n] bool, start state 0.  Trimmed: from every state an accepting state is reachable, so a byte
    string is a live prefix exactly while walk() does not return -1."""

    def __init__(self, trans, accept, pattern=""):
        self.trans, self.accept, self.pattern = trans, accept, pattern
        self.n = trans.shape[0]

    def walk(self, data: bytes, state: int = 0) -> int:
        for b in data:
            if state < 0:
                return -1
            state = int(self.trans[state, b])
        return state

    def accepts(self, data: bytes) -> bool:
        s = self.walk(data)
        return s >= 0 and bool(self.accept[s])

    def live(self, data: bytes) -> bool:
        return self.walk(data) >= 0


def compile_regex(pattern: str) -> ByteDFA:
    tree = _Parser(pattern).parse()
    nfa = _NFA()
    entry, exit_ = nfa.build(tree)
    # subset construction
    closures = {}

    def closure(states):
        key = frozenset(states)
        got = closures.get(key)
        if got is None:
            seen, stack = set(key), list(key)
            while stack:
                for t in nfa.eps[stack.pop()]:
                    if t not in seen:
                        seen.add(t)
                        stack.append(t)
            got = closures[key] = frozenset(seen)
        return got

    start = closure([entry])
    index, order, rows = {start: 0}, [start], []
    k = 0
    while k < len(order):
        edges = [nfa.edge[s] for s in order[k] if nfa.edge[s] is not None]
        row = np.full(256, -1, dtype=np.int32)
        by_targets = {}
        for byte in range(256):
            tg = tuple(t for m, t in edges if (m >> byte) & 1)
            if tg:
                by_targets.setdefault(tg, []).append(byte)
        for tg, bts in by_targets.items():
            nxt = closure(tg)
            j = index.get(nxt)
            if j is None:
                j = index[nxt] = len(order)
                order.append(nxt)
            row[bts] = j
        rows.append(row)
        k += 1
    trans = np.stack(rows)
    accept = np.array([exit_ in st for st in order], dtype=bool)
    # trim: states that cannot reach acceptance go, transitions into them become -1
    n = len(order)
    live = accept.copy()
    while True:
        reach = np.concatenate([live, [False]])[trans].any(1) | live      # (index -1 reads the appended False)
        if (reach == live).all():
            break
        live = reach
    if not live[0]:                       # the empty language: one state, nothing allowed, nothing accepted
        return ByteDFA(np.full((1, 256), -1, dtype=np.int32), np.zeros(1, dtype=bool), pattern)
    trans = np.where(np.concatenate([live, [False]])[trans], trans, -1)
    # Moore partition refinement over the live states (dead ones keep block -1 through the extended lookup)
    block = np.where(live, accept.astype(np.int64), -1)
    count = len(np.unique(block[live]))
    while True:             # a state's signature holds its own block, so every round refines the partition: it is stable when the block count stops growing
        ext = np.concatenate([block, [-1]])
        sig = np.concatenate([block[:, None], ext[trans]], 1)
        _, inv = np.unique(sig[live], axis=0, return_inverse=True)
        block = np.full(n, -1, dtype=np.int64)
        block[live] = inv.reshape(-1)
        if int(inv.max()) + 1 == count:
            break
        count = int(inv.max()) + 1
    # renumber in breadth-first order from the start, so that the result does not depend on numpy's sort order
    rep = {}
    for s in range(n):
        if live[s]:
            rep.setdefault(int(block[s]), s)
    number, queue = {int(block[0]): 0}, [int(block[0])]
    out_rows = []
    k = 0
    while k < len(queue):
        row = trans[rep[queue[k]]]
        new_row = np.full(256, -1, dtype=np.int32)
        for byte in range(256):
            t = int(row[byte])
            if t >= 0:
                bl = int(block[t])
                if bl not in number:
                    number[bl] = len(queue)
                    queue.append(bl)
                new_row[byte] = number[bl]
        out_rows.append(new_row)
        k += 1
    return ByteDFA(np.stack(out_rows), np.array([bool(accept[rep[b]]) for b in queue], dtype=bool), pattern)


# ---- tokenizer -> bytes ----------------------------------------------------------------------------------------------------------------------------------------

def _gpt2_unicode_to_byte():
    """The inverse of GPT-2's bytes_to_unicode: printable bytes stand for themselves, the other 68 are moved to U+0100 onwards."""
    keep = list(range(ord("!"), ord("~") + 1)) + list(range(0xA1, 0xAD)) + list(range(0xAE, 0x100))
    table, n = {chr(b): b for b in keep}, 0
    for b in range(256):
        if b not in keep:
            table[chr(256 + n)] = b
            n += 1
    return table


def _types_in(node):
    """The "type" names of a tokenizers JSON component and of everything nested in it (Sequence)."""
    if not isinstance(node, dict):
        return []
    out = [node.get("type")]
    for key in ("decoders", "pretokenizers"):
        for sub in node.get(key) or []:
            out += _types_in(sub)
    return [t for t in out if t]


def token_bytes(tokenizer, vocab_size: int) -> list:
    """The byte string of every id in [0, vocab_size), None for ids that may never be emitted: special and added tokens, ids the tokenizer does not have (between
    len(tokenizer) and the model's padded vocab_size) and tokens that stand for no bytes at all.  `tokenizer`: a transformers fast tokenizer or a tokenizers.Tokenizer.
      byte-level BPE (Qwen): a ByteLevel decoder or pre-tokenizer -- every character of the token string through GPT-2's unicode-to-byte map;
      sentencepiece-style (LLaVA): a Metaspace decoder, or a vocabulary with U+2581 / <0xNN> tokens -- U+2581 is a space, <0xNN> is that byte, the rest UTF-8
        (the decoder's stripping of one leading space at the start of a text is not modelled: a pattern sees the space);
      no decoder at all (WordLevel character tokenizers): the token string in UTF-8.
    Any other decoder is refused by name."""
    backend = getattr(tokenizer, "backend_tokenizer", tokenizer)
    if not hasattr(backend, "to_str") or not hasattr(backend, "get_vocab"):
        raise ValueError(f"token_bytes needs a fast tokenizer (tokenizers backend), got {type(tokenizer).__name__}")
    spec = json.loads(backend.to_str())
    dec, pre = _types_in(spec.get("decoder")), _types_in(spec.get("pre_tokenizer"))
    vocab = backend.get_vocab(with_added_tokens=True)
    never = set(int(i) for i in backend.get_added_tokens_decoder())
    never |= set(int(i) for i in (getattr(tokenizer, "all_special_ids", None) or []))
    regular = [t for t, i in vocab.items() if i not in never]
    if "ByteLevel" in dec or "ByteLevel" in pre:
        table = _gpt2_unicode_to_byte()

        def conv(tok):
            try:
                return bytes(table[ch] for ch in tok)
            except KeyError:
                raise ValueError(f"byte-level tokenizer with a token outside the GPT-2 byte alphabet: {tok!r}") from None
    elif "Metaspace" in dec or any("▁" in t for t in regular) or any(len(t) == 6 and t.startswith("<0x") and t.endswith(">") for t in regular):
        def conv(tok):
            if len(tok) == 6 and tok.startswith("<0x") and tok.endswith(">"):
                try:
                    return bytes([int(tok[3:5], 16)])
                except ValueError:
                    pass
            return tok.replace("▁", " ").encode("utf-8")
    elif not dec:
        def conv(tok):
            return tok.encode("utf-8")
    else:
        raise ValueError(f"token_bytes: no byte rule for a tokenizer whose decoder is {' + '.join(dec)} (known: ByteLevel, Metaspace / U+2581 vocabularies, no decoder)")
    out = [None] * int(vocab_size)
    for tok, i in vocab.items():
        if 0 <= i < vocab_size and i not in never:
            b = conv(tok)
            out[i] = b if b else None
    return out


# ---- byte DFA x vocabulary -> the sampler's tables -----------------------------------------------------------------------------------------------------------

class TokenGuide:
    """allow [S, ceil(V / 32)] uint32 (bit id & 31 of word id >> 5: token id may follow state s) and trans [S, V] int16 (the state behind (s, id), -1 where not
    allowed); state 0 is the start.  Two tables because the sampler streams a row of `allow` every step (19 KB at V = 151936) and touches ONE element of `trans`,
    whose row is 300 KB.  Built by build() only."""

    def __init__(self, allow, trans, accepting, byte_state, dfa, eos_id, build_seconds):
        self.allow, self.trans, self.accepting, self.byte_state, self.dfa, self.eos_id = allow, trans, accepting, byte_state, dfa, int(eos_id)
        self.S, self.V = trans.shape
        self.start = 0
        self.pattern = dfa.pattern
        self.build_seconds = build_seconds
        self._dev = {}          # device -> (allow, trans) uploaded once (Rollout.generate)

    @property
    def nbytes(self) -> int:
        return int(self.allow.nbytes + self.trans.nbytes)

    def walk(self, ids, state: int = 0) -> int:
        """The state after emitting ids from `state`, -1 as soon as one of them is not allowed."""
        for t in ids:
            if state < 0 or not (0 <= int(t) < self.V):
                return -1
            state = int(self.trans[state, int(t)])
        return state

    def device_tables(self, device):
        import torch
        key = str(device)
        if key not in self._dev:
            self._dev[key] = (torch.from_numpy(self.allow.view(np.int32)).to(device), torch.from_numpy(self.trans).to(device))
        return self._dev[key]

    @staticmethod
    def build(dfa: ByteDFA, token_bytes: list, eos_id: int, vocab_size: int) -> "TokenGuide":
        t0 = time.perf_counter()
        V, S0 = int(vocab_size), dfa.n
        if len(token_bytes) != V:
            raise ValueError(f"token_bytes has {len(token_bytes)} entries for vocab_size {V}")
        if not (0 <= int(eos_id) < V):
            raise ValueError(f"eos_id {eos_id} outside the vocabulary [0, {V})")
        W = (V + 31) // 32
        nbytes = S0 * (V * 2 + W * 4)
        if S0 > MAX_STATES or nbytes > MAX_TABLE_BYTES:
            raise ValueError(f"guide tables too large: S = {S0} states (limit {MAX_STATES}) x V = {V} tokens = {nbytes} bytes (limit {MAX_TABLE_BYTES}); simplify the pattern")
        # tokens sorted by length: at byte position j only a suffix of them is still being walked
        ids = np.array([i for i, b in enumerate(token_bytes) if b and i != eos_id], dtype=np.int64)
        lens = np.array([len(token_bytes[i]) for i in ids], dtype=np.int64)
        order = np.argsort(lens, kind="stable")
        ids, lens = ids[order], lens[order]
        T, L = len(ids), int(lens.max()) if len(ids) else 0
        tb = np.zeros((T, max(L, 1)), dtype=np.uint8)
        for r, i in enumerate(ids):
            tb[r, : lens[r]] = np.frombuffer(token_bytes[i], dtype=np.uint8)
        first = np.searchsorted(lens, np.arange(L) + 1, side="left")      # first[j]: the first token longer than j bytes
        step = np.concatenate([dfa.trans, np.full((1, 256), -1, dtype=np.int32)])   # row -1: dead stays dead
        trans = np.full((S0, V), -1, dtype=np.int16)
        BLK = max(1, (1 << 24) // max(T, 1))
        for s0 in range(0, S0, BLK):
            cur = np.repeat(np.arange(s0, min(S0, s0 + BLK), dtype=np.int32)[:, None], T, 1)
            for j in range(L):
                k = first[j]
                cur[:, k:] = step[cur[:, k:], tb[k:, j][None, :]]
            trans[s0: s0 + BLK, ids] = cur
        acc = dfa.accept
        trans[:, eos_id] = np.where(acc, np.arange(S0), -1)              # EOS exactly where the bytes so far match; a finished row idles in place
        # token-level pruning to a fixpoint: good = acceptance reachable BY TOKENS; transitions into the other states go
        succ = [np.unique(r[r >= 0]) for r in trans]
        good = acc.copy()
        while True:
            new = good | np.array([bool(good[u].any()) for u in succ])
            if (new == good).all():
                break
            good = new
        if not good[0]:
            raise ValueError(f"the pattern {dfa.pattern!r} cannot be completed with this vocabulary: no token sequence from the start reaches a match")
        trans[~np.concatenate([good, [False]])[trans]] = -1
        # keep the states tokens can reach from the start, renumbered breadth-first (start = 0)
        number, queue = {0: 0}, [0]
        k = 0
        while k < len(queue):
            r = trans[queue[k]]
            for u in np.unique(r[r >= 0]):
                if int(u) not in number:
                    number[int(u)] = len(queue)
                    queue.append(int(u))
            k += 1
        remap = np.full(S0 + 1, -1, dtype=np.int16)
        remap[queue] = np.arange(len(queue), dtype=np.int16)
        trans = np.ascontiguousarray(remap[trans[queue]])
        if not (trans >= 0).any(1).all():
            raise ValueError(f"the pattern {dfa.pattern!r} cannot be completed with this vocabulary: a reachable state allows no token")
        bits = np.packbits(trans >= 0, axis=1, bitorder="little")
        padded = np.zeros((len(queue), W * 4), dtype=np.uint8)
        padded[:, : bits.shape[1]] = bits
        allow = padded.view("<u4").astype(np.uint32)
        return TokenGuide(allow, trans, acc[queue].copy(), np.array(queue, dtype=np.int32), dfa, eos_id, time.perf_counter() - t0)


def build_guide(pattern: str, tokenizer, eos_id: int, vocab_size: int) -> TokenGuide:
    """compile_regex -> token_bytes -> TokenGuide.build; build_seconds covers all three."""
    t0 = time.perf_counter()
    g = TokenGuide.build(compile_regex(pattern), token_bytes(tokenizer, vocab_size), eos_id, vocab_size)
    g.build_seconds = time.perf_counter() - t0
    return g
