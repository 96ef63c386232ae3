"""Host side of guided decoding: a regular expression (or a choice list, which is one) compiled to a byte-level DFA, the
vocabulary's byte table, the liveness check of a DFA against a vocabulary, and a plain NumPy restatement of the device rule.

The rule itself is written out in include/p3v.h above `p3v_guide_row_t`; the kernel in csrc/p3v_guide.hip implements it and
`reference_mask` here reproduces every output bit and every state.

A guide is a DFA over BYTES: states 1..S (S <= 255), state 0 dead, state 1 the start, `delta` uint16 [S + 1, 256], `accept`
uint8 [S + 1].  It constrains the UTF-8 bytes of the whole output (full-match semantics): the concatenated byte strings of the
generated token ids up to EOS.  EOS is allowed exactly in accepting states; `max_tokens` can still cut the output before the
pattern completes.

The regex subset: literals (non-ASCII characters as their UTF-8 bytes), `.` and negated classes (exactly one well-formed UTF-8
code point not excluded; `.` excludes \\n), classes with ASCII members and ranges, \\d \\w \\s \\D \\W \\S with ASCII meaning,
\\n \\t \\r \\f \\v \\0 \\xHH and escaped metacharacters, * + ? {m} {m,} {m,n} {,n}, ( ), (?: ) and |.  Anchors, back-references,
look-around, named groups, inline flags, lazy and possessive quantifiers and a non-ASCII class member raise ValueError naming the
construct.  The oracle the tests hold this to is Python's re.fullmatch(pattern, s, re.ASCII).

No third-party library: the Thompson construction, the subset construction, the minimisation and the pruning are below.
"""
import re as _re
from collections import OrderedDict

import numpy as np

MAX_STATES = 255                      # P3V_GUIDE_MAX_STATES
DONE = -1                             # p3v_guide_row_t.state after EOS
ACTIVE = 1                            # P3V_GUIDE_ACTIVE (bit 0 of flags)
RECORD_WORDS = 4                      # sizeof(p3v_guide_row_t) / 4: {flags, n_states, state, reserved}
NEG_INF = 0xFF80                      # bf16 -inf
_SUBSET_CAP = 20000                   # subset construction gives up beyond this many DFA states

_DIGIT = frozenset(range(0x30, 0x3A))
_WORD = frozenset(list(range(0x30, 0x3A)) + list(range(0x41, 0x5B)) + list(range(0x61, 0x7B)) + [0x5F])
_SPACE = frozenset(b" \t\n\r\f\v")
_ASCII = frozenset(range(128))
_META = set("\\.^$*+?{}[]|()")
_SIMPLE_ESC = {"n": 10, "t": 9, "r": 13, "f": 12, "v": 11, "a": 7, "0": 0}


class Dfa:
    """A compiled guide: delta uint16 [S + 1, 256] (row 0 all zero), accept uint8 [S + 1] (accept[0] == 0), n_states S."""

    def __init__(self, delta, accept, pattern=None):
        self.delta = np.ascontiguousarray(delta, dtype=np.uint16)
        self.accept = np.ascontiguousarray(accept, dtype=np.uint8)
        self.n_states = int(self.delta.shape[0]) - 1
        self.pattern = pattern

    def walk(self, data, state=1):
        for b in bytes(data):
            if state == 0:
                break
            state = int(self.delta[state, b])
        return state

    def matches(self, data):
        """Full match of a str (its UTF-8 bytes) or a bytes object."""
        data = data.encode("utf-8") if isinstance(data, str) else data
        return bool(self.accept[self.walk(data)])


# ----------------------------------------------------------------------------- parser: pattern -> AST
# AST nodes: ("set", frozenset of bytes) | ("anycp", frozenset of excluded ASCII bytes, ascii_allowed) | ("cat", [nodes]) |
# ("alt", [nodes]) | ("rep", node, m, n or None) | ("eps",)
class _Parser:
    def __init__(self, pattern):
        if not isinstance(pattern, str):
            raise ValueError(f"a guide pattern must be a string, got {type(pattern).__name__}")
        self.p, self.i = pattern, 0

    def fail(self, what):
        raise ValueError(f"guided_regex: unsupported construct {what} at position {self.i} of {self.p!r}")

    def peek(self):
        return self.p[self.i] if self.i < len(self.p) else None

    def parse(self):
        node = self.alt()
        if self.i < len(self.p):
            self.fail("unbalanced ')'")
        return node

    def alt(self):
        branches = [self.cat()]
        while self.peek() == "|":
            self.i += 1
            branches.append(self.cat())
        return branches[0] if len(branches) == 1 else ("alt", branches)

    def cat(self):
        items = []
        while self.peek() is not None and self.peek() not in "|)":
            items.append(self.quantified())
        return ("cat", items) if items else ("eps",)

    def quantified(self):
        atom = self.atom()
        while True:
            c = self.peek()
            if c == "*":
                m, n = 0, None
            elif c == "+":
                m, n = 1, None
            elif c == "?":
                m, n = 0, 1
            elif c == "{":
                mt = _re.compile(r"\{(\d*)(,(\d*))?\}").match(self.p, self.i)
                if mt is None or (mt.group(1) == "" and mt.group(2) is None):
                    return atom                                 # (not a quantifier: '{' is a literal, as in `re`)
                m = int(mt.group(1) or 0)
                n = m if mt.group(2) is None else (int(mt.group(3)) if mt.group(3) else None)
                if n is not None and n < m:
                    raise ValueError(f"guided_regex: bad repeat {mt.group(0)!r} (min > max) in {self.p!r}")
                self.i = mt.end() - 1
            else:
                return atom
            self.i += 1
            if self.peek() == "?":
                self.fail("lazy quantifier")
            if self.peek() == "+":
                self.fail("possessive quantifier")
            if self.peek() in ("*",) or (self.peek() == "{" and _re.compile(r"\{\d*(,\d*)?\}").match(self.p, self.i)):
                self.fail("multiple repeat")
            atom = ("rep", atom, m, n)

    def atom(self):
        c = self.peek()
        self.i += 1
        if c == "(":
            if self.peek() == "?":
                nxt = self.p[self.i + 1:self.i + 3]
                if nxt[:1] == ":":
                    self.i += 2
                elif nxt[:1] in ("=", "!") or nxt[:2] in ("<=", "<!"):
                    self.fail("look-around")
                elif nxt[:1] == "P" or nxt[:1] == "<":
                    self.fail("named group / back-reference")
                else:
                    self.fail("group extension '(?" + nxt[:1] + "'")
            node = self.alt()
            if self.peek() != ")":
                self.fail("unbalanced '('")
            self.i += 1
            return node
        if c == "[":
            return self.klass()
        if c == ".":
            return ("anycp", frozenset([10]), True)
        if c in "^$":
            self.i -= 1
            self.fail(f"anchor {c!r}")
        if c in "*+?":
            self.i -= 1
            self.fail("nothing to repeat")
        if c == ")":
            self.i -= 1
            self.fail("unbalanced ')'")
        if c == "\\":
            kind, val = self.escape(in_class=False)
            if kind == "lit":
                return _literal(chr(val))
            ascii_set, nonascii = val
            return ("anycp", _ASCII - ascii_set, True) if nonascii else ("set", ascii_set)
        return _literal(c)

    def escape(self, in_class):
        """After a backslash: ("lit", code point) or ("cls", (frozenset of ASCII bytes, includes every non-ASCII code point))."""
        c = self.peek()
        if c is None:
            self.fail("trailing backslash")
        self.i += 1
        if c in "dws":
            return "cls", ({"d": _DIGIT, "w": _WORD, "s": _SPACE}[c], False)
        if c in "DWS":
            return "cls", (_ASCII - {"D": _DIGIT, "W": _WORD, "S": _SPACE}[c], True)
        if c == "x":
            h = self.p[self.i:self.i + 2]
            if len(h) != 2 or any(ch not in "0123456789abcdefABCDEF" for ch in h):
                self.fail("incomplete \\x escape")
            self.i += 2
            return "lit", int(h, 16)
        if c == "0" and not (self.peek() or "x").isdigit():
            return "lit", 0
        if c.isdigit():
            self.i -= 1
            self.fail(f"back-reference or octal escape \\{c}")
        if c == "b" and in_class:
            return "lit", 8
        if c in "AZbB":
            self.i -= 1
            self.fail(f"anchor \\{c}")
        if c in _SIMPLE_ESC:
            return "lit", _SIMPLE_ESC[c]
        if c.isascii() and c.isalpha():
            self.i -= 1
            self.fail(f"escape \\{c}")
        return "lit", ord(c)                                    # an escaped metacharacter or punctuation

    def klass(self):
        negate = self.peek() == "^"
        if negate:
            self.i += 1
        members, nonascii, first = set(), False, True
        while True:
            c = self.peek()
            if c is None:
                self.fail("unterminated character class")
            if c == "]" and not first:
                self.i += 1
                break
            first = False
            lo = self.class_atom()
            if isinstance(lo, tuple):                           # a shorthand class: no range
                members |= lo[0]
                nonascii = nonascii or lo[1]
                continue
            if self.peek() == "-" and self.p[self.i + 1:self.i + 2] not in ("]", ""):
                self.i += 1
                hi = self.class_atom()
                if isinstance(hi, tuple):
                    self.fail("range with a class shorthand")
                if hi < lo:
                    raise ValueError(f"guided_regex: bad character range in {self.p!r}")
                members |= set(range(lo, hi + 1))
            else:
                members.add(lo)
        members = frozenset(members)
        if negate:
            return ("set", _ASCII - members) if nonascii else ("anycp", members, True)
        return ("anycp", _ASCII - members, True) if nonascii else ("set", members)

    def class_atom(self):
        c = self.peek()
        self.i += 1
        if c == "\\":
            kind, val = self.escape(in_class=True)
            if kind == "cls":
                return val
            cp = val
        else:
            cp = ord(c)
        if cp > 127:
            self.i -= 1
            self.fail(f"non-ASCII class member {chr(cp)!r}")
        return cp


def _literal(ch):
    bs = ch.encode("utf-8")
    return ("set", frozenset([bs[0]])) if len(bs) == 1 else ("cat", [("set", frozenset([b])) for b in bs])


def _r(lo, hi):
    return ("set", frozenset(range(lo, hi + 1)))


_CONT = _r(0x80, 0xBF)
# every well-formed UTF-8 sequence of two to four bytes (no overlongs, no surrogates, nothing above U+10FFFF)
_MULTIBYTE = [("cat", [_r(0xC2, 0xDF), _CONT]),
              ("cat", [_r(0xE0, 0xE0), _r(0xA0, 0xBF), _CONT]), ("cat", [_r(0xE1, 0xEC), _CONT, _CONT]),
              ("cat", [_r(0xED, 0xED), _r(0x80, 0x9F), _CONT]), ("cat", [_r(0xEE, 0xEF), _CONT, _CONT]),
              ("cat", [_r(0xF0, 0xF0), _r(0x90, 0xBF), _CONT, _CONT]), ("cat", [_r(0xF1, 0xF3), _CONT, _CONT, _CONT]),
              ("cat", [_r(0xF4, 0xF4), _r(0x80, 0x8F), _CONT, _CONT])]


# ----------------------------------------------------------------------------- Thompson construction: AST -> NFA over bytes
class _Nfa:
    def __init__(self):
        self.eps = []                                           # state -> [states]
        self.edges = []                                         # state -> [(frozenset of bytes, state)]

    def new(self):
        self.eps.append([])
        self.edges.append([])
        if len(self.eps) > 200000:
            raise ValueError("guided_regex: the pattern expands to more than 200000 NFA states")
        return len(self.eps) - 1

    def build(self, node):
        """-> (entry, exit) of the fragment for `node`."""
        kind = node[0]
        a, b = self.new(), self.new()
        if kind == "eps":
            self.eps[a].append(b)
        elif kind == "set":
            self.edges[a].append((node[1], b))
        elif kind == "anycp":
            allowed = _ASCII - node[1]
            if allowed:
                self.edges[a].append((frozenset(allowed), b))
            for seq in _MULTIBYTE:
                s, e = self.build(seq)
                self.eps[a].append(s)
                self.eps[e].append(b)
        elif kind == "cat":
            cur = a
            for item in node[1]:
                s, e = self.build(item)
                self.eps[cur].append(s)
                cur = e
            self.eps[cur].append(b)
        elif kind == "alt":
            for item in node[1]:
                s, e = self.build(item)
                self.eps[a].append(s)
                self.eps[e].append(b)
        elif kind == "rep":
            _, item, m, n = node
            cur = a
            for _ in range(m):
                s, e = self.build(item)
                self.eps[cur].append(s)
                cur = e
            if n is None:                                       # a star behind the m copies
                s, e = self.build(item)
                hub = self.new()
                self.eps[cur].append(hub)
                self.eps[hub].append(s)
                self.eps[e].append(hub)
                cur = hub
            else:                                               # n - m optional copies, each skipping to the end
                for _ in range(n - m):
                    s, e = self.build(item)
                    self.eps[cur].append(s)
                    self.eps[cur].append(b)
                    cur = e
            self.eps[cur].append(b)
        else:
            raise AssertionError(kind)
        return a, b

    def closure(self, states):
        seen, stack = set(states), list(states)
        while stack:
            for t in self.eps[stack.pop()]:
                if t not in seen:
                    seen.add(t)
                    stack.append(t)
        return frozenset(seen)


# ----------------------------------------------------------------------------- subset construction, minimisation, pruning
def _subset(nfa, start, final):
    """-> (delta int32 [N, 256] complete over N subsets, subset 0 = the start; accept bool [N])."""
    s0 = nfa.closure([start])
    index, order, rows = {s0: 0}, [s0], []
    k = 0
    while k < len(order):
        cur = order[k]
        k += 1
        by_byte = {}
        for s in cur:
            for bs, t in nfa.edges[s]:
                for b in bs:
                    by_byte.setdefault(b, set()).add(t)
        row = np.full(256, -1, dtype=np.int64)
        memo = {}
        for b, ts in by_byte.items():
            key = frozenset(ts)
            if key not in memo:
                nxt = nfa.closure(key)
                if nxt not in index:
                    index[nxt] = len(order)
                    order.append(nxt)
                    if len(order) > _SUBSET_CAP:
                        raise ValueError(f"guided_regex: more than {_SUBSET_CAP} states in the subset construction "
                                         f"(a guide holds at most {MAX_STATES})")
                memo[key] = index[nxt]
            row[b] = memo[key]
        rows.append(row)
    delta = np.stack(rows)
    dead = len(order)                                           # one explicit dead state completes the table
    delta = np.concatenate([np.where(delta < 0, dead, delta), np.full((1, 256), dead, dtype=np.int64)])
    accept = np.array([final in s for s in order] + [False])
    return delta, accept


def _minimise(delta, accept):
    """Moore's partition refinement on a complete DFA -> (class of every state, number of classes)."""
    cls = accept.astype(np.int64)
    n_cls = len(np.unique(cls))
    while True:
        sig = np.concatenate([cls[:, None], cls[delta]], axis=1)
        _, new = np.unique(sig, axis=0, return_inverse=True)
        new = new.reshape(-1)
        n_new = int(new.max()) + 1
        if n_new == n_cls:
            return new, n_new
        cls, n_cls = new, n_new


def _finish(delta, accept, pattern):
    cls, n = _minimise(delta, accept)
    rep = np.zeros(n, dtype=np.int64)
    rep[cls[::-1]] = np.arange(len(cls))[::-1]                  # one member per class
    mdelta, maccept = cls[delta[rep]], accept[rep]
    # pruning: the classes that cannot reach an accepting one are the dead state (after minimisation: at most one class)
    live = maccept.copy()
    while True:
        grown = live | live[mdelta].any(axis=1)
        if (grown == live).all():
            break
        live = grown
    start = int(cls[0])
    if not live[start]:
        raise ValueError(f"guided_regex: {pattern!r} matches nothing")
    # renumber: 0 dead, 1 the start, the rest in breadth-first order from the start
    number, queue = {start: 1}, [start]
    for s in queue:
        for t in mdelta[s]:
            t = int(t)
            if live[t] and t not in number:
                number[t] = len(number) + 1
                queue.append(t)
    S = len(number)
    if S > MAX_STATES:
        raise ValueError(f"guided_regex: {pattern!r} needs {S} states after minimisation; a guide holds at most {MAX_STATES}")
    out = np.zeros((S + 1, 256), dtype=np.uint16)
    acc = np.zeros(S + 1, dtype=np.uint8)
    for s, k in number.items():
        row = mdelta[s]
        out[k] = [number[int(t)] if live[t] else 0 for t in row]
        acc[k] = 1 if maccept[s] else 0
    return Dfa(out, acc, pattern)


def _compile(pattern):
    ast = _Parser(pattern).parse()
    nfa = _Nfa()
    start, final = nfa.build(ast)
    return _finish(*_subset(nfa, start, final), pattern)


# ----------------------------------------------------------------------------- the host LRU cache of compiled guides
CACHE_SIZE = 64
_cache = OrderedDict()


def compile_regex(pattern):
    """The minimised, pruned DFA of `pattern` (full-match semantics over UTF-8 bytes); ValueError names an unsupported construct
    or the state count beyond 255.  Compiled guides are kept in a small LRU cache keyed by the pattern."""
    if not isinstance(pattern, str):
        raise ValueError(f"guided_regex must be a string, got {type(pattern).__name__}")
    hit = _cache.get(pattern)
    if hit is not None:
        _cache.move_to_end(pattern)
        return hit
    dfa = _compile(pattern)
    _cache[pattern] = dfa
    while len(_cache) > CACHE_SIZE:
        _cache.popitem(last=False)
    return dfa


def escape(text):
    """`text` as a pattern of this subset that matches exactly it."""
    return "".join("\\" + c if c in _META else {"\n": "\\n", "\t": "\\t", "\r": "\\r"}.get(c, c) for c in text)


def compile_choice(choices):
    """A choice list: the alternation of its escaped literals, through the same compiler."""
    if isinstance(choices, (str, bytes)) or not isinstance(choices, (list, tuple)) or not choices:
        raise ValueError("guided_choice must be a non-empty list of strings")
    for c in choices:
        if not isinstance(c, str):
            raise ValueError(f"guided_choice must be a non-empty list of strings, got an element of type {type(c).__name__}")
    return compile_regex("|".join("(?:" + escape(c) + ")" for c in choices))


def compile_guide(regex=None, choice=None):
    """One request's guide: None when it asks for none; both at once raise."""
    if regex is not None and choice is not None:
        raise ValueError("guided_regex and guided_choice exclude each other: give one per prompt")
    if regex is not None:
        return compile_regex(regex)
    if choice is not None:
        return compile_choice(choice)
    return None


def per_prompt(B, regex=None, choice=None):
    """The public arguments -- each one value for every prompt, or a list of one value / None per prompt -- as B compiled
    guides / None, or None when no prompt has one.  (A choice list is a list of strings: a per-prompt list of choices is a
    list of lists / None.)"""
    if isinstance(regex, (list, tuple)):
        if len(regex) != B:
            raise ValueError(f"guided_regex: {len(regex)} values for {B} prompts")
        rx = list(regex)
    else:
        rx = [regex] * B
    if isinstance(choice, (list, tuple)) and choice and all(c is None or isinstance(c, (list, tuple)) for c in choice):
        if len(choice) != B:
            raise ValueError(f"guided_choice: {len(choice)} values for {B} prompts")
        ch = list(choice)
    else:
        ch = [choice] * B
    out = [compile_guide(r, c) for r, c in zip(rx, ch)]
    return None if all(g is None for g in out) else out


def refuse_speculation(guides, speculate):
    if guides is not None and speculate and any(g is not None for g in guides):
        raise ValueError("speculate: guided decoding is not supported (a verify step scores several tokens per replay "
                         "against one guide state; speculate must be 0)")


# ----------------------------------------------------------------------------- the vocabulary table
class VocabTable:
    """tok_off uint32 [n + 1], tok_bytes uint8 [tok_off[n]] (at least one byte is allocated): the byte string of every id."""

    def __init__(self, strings):
        lens = np.fromiter((len(s) for s in strings), dtype=np.int64, count=len(strings))
        self.n = len(strings)
        self.tok_off = np.zeros(self.n + 1, dtype=np.uint32)
        self.tok_off[1:] = np.cumsum(lens)
        self.tok_bytes = np.frombuffer(b"".join(strings) or b"\0", dtype=np.uint8).copy()
        self.n_bytes = int(self.tok_off[-1])
        self._padded = None

    def bytes_of(self, i):
        return self.tok_bytes[int(self.tok_off[i]):int(self.tok_off[i + 1])].tobytes()

    def padded(self):
        """(lengths int64 [n], bytes uint8 [n, longest]) for the vectorised walk."""
        if self._padded is None:
            off = self.tok_off.astype(np.int64)
            lens = off[1:] - off[:-1]
            width = max(int(lens.max()) if self.n else 0, 1)
            mat = np.zeros((self.n, width), dtype=np.uint8)
            col = np.arange(width)[None, :]
            sel = col < lens[:, None]
            mat[sel] = self.tok_bytes[:self.n_bytes]
            self._padded = (lens, mat)
        return self._padded


_BYTE_PIECE = _re.compile(r"<0x([0-9A-Fa-f]{2})>\Z")


def token_bytes(tokenizer, vocab_size):
    """The vocabulary table of a tokenizer over ids [0, vocab_size).  ByteTokenizer: ids 3..258 are one byte each, everything
    else is empty.  A sentencepiece-style tokenizer (convert_ids_to_tokens): a piece's `▁` is a space, `<0xHH>` is that
    byte, special tokens, ids beyond the tokenizer's own vocabulary and ids it has no piece for are empty."""
    n = int(vocab_size)
    if n < 1:
        raise ValueError(f"token_bytes: vocab_size must be >= 1, got {vocab_size}")
    strings = [b""] * n
    if type(tokenizer).__name__ == "ByteTokenizer":
        for i in range(3, min(259, n)):
            strings[i] = bytes([i - 3])
        return VocabTable(strings)
    if not hasattr(tokenizer, "convert_ids_to_tokens"):
        raise ValueError(f"token_bytes: {type(tokenizer).__name__} has no convert_ids_to_tokens")
    try:
        own = len(tokenizer)
    except TypeError:
        own = int(getattr(tokenizer, "vocab_size", n))
    special = set(getattr(tokenizer, "all_special_ids", None) or [])
    special_txt = set(getattr(tokenizer, "all_special_tokens", None) or [])
    ids = list(range(min(n, own)))
    pieces = tokenizer.convert_ids_to_tokens(ids)
    for i, piece in zip(ids, pieces):
        if piece is None or i in special or piece in special_txt:
            continue
        m = _BYTE_PIECE.match(piece)
        strings[i] = bytes([int(m.group(1), 16)]) if m else piece.replace("▁", " ").encode("utf-8")
    return VocabTable(strings)


_tables = OrderedDict()


def vocab_for(tokenizer, vocab_size):
    """The vocabulary table of a tokenizer, built once per (tokenizer, size) and kept while the tokenizer lives here."""
    key = (id(tokenizer), int(vocab_size))
    hit = _tables.get(key)
    if hit is not None and hit[0] is tokenizer:
        return hit[1]
    table = token_bytes(tokenizer, vocab_size)
    _tables[key] = (tokenizer, table)
    while len(_tables) > 8:
        _tables.popitem(last=False)
    return table


def replay_state(dfa, table, fed, eos):
    """The state of a row that started at state 1 and was fed the ids `fed` in order (the rule's step 1, on the host)."""
    if dfa is None:
        return 0
    state = 1
    for f in fed:
        f = int(f)
        if state == DONE:
            break
        if f == int(eos):
            state = DONE
        elif 0 <= f < table.n:
            bs = table.bytes_of(f)
            if bs:
                state = dfa.walk(bs, state)
                if state == 0:
                    break
    return state


def _walk_all(delta, states, lens, mat, n_states):
    """walk(states[i], bytes(i)) for every token: delta [*, 256] with entries above n_states counting as dead."""
    s = np.array(states, dtype=np.int64)
    for k in range(mat.shape[1]):
        go = (lens > k) & (s > 0)
        if not go.any():
            break
        nxt = delta[s[go], mat[go, k]].astype(np.int64)
        nxt[nxt > n_states] = 0
        s[go] = nxt
    return s


def check(dfa, table, eos):
    """The compile-time liveness check against a vocabulary: every state 1..S either accepts (EOS is then allowed; `eos` must lie
    in the table) or allows at least one token.  ValueError names the first state that does neither."""
    lens, mat = table.padded()
    if not 0 <= int(eos) < table.n:
        raise ValueError(f"guide check: eos id {eos} lies outside the vocabulary [0, {table.n})")
    has = lens > 0
    has[int(eos)] = False
    for s in range(1, dfa.n_states + 1):
        if dfa.accept[s]:
            continue
        end = _walk_all(dfa.delta, np.full(table.n, s), lens, mat, dfa.n_states)
        if not ((end > 0) & has).any():
            raise ValueError(f"guide {dfa.pattern!r}: no token of the vocabulary continues from state {s} and it does not accept "
                             "(this vocabulary cannot spell the pattern)")


_checked = OrderedDict()


def checked(dfa, table, eos):
    """`check` once per (guide, table): a small LRU cache beside the compiled guides."""
    key = (id(dfa), id(table), int(eos))
    if key in _checked and _checked[key][0] is dfa and _checked[key][1] is table:
        _checked.move_to_end(key)
        return dfa
    check(dfa, table, eos)
    _checked[key] = (dfa, table)
    while len(_checked) > 4 * CACHE_SIZE:
        _checked.popitem(last=False)
    return dfa


# ----------------------------------------------------------------------------- records and the rule in NumPy
def record(dfa, state=1):
    """One row's p3v_guide_row_t words: an inactive row for None."""
    return [0, 0, 0, 0] if dfa is None else [ACTIVE, dfa.n_states, int(state), 0]


def region(dfa):
    """A guide as one row's table region: (delta uint16 [256, 256], accept uint8 [256]), zero beyond its states."""
    d = np.zeros((256, 256), dtype=np.uint16)
    a = np.zeros(256, dtype=np.uint8)
    d[:dfa.n_states + 1] = dfa.delta
    a[:dfa.n_states + 1] = dfa.accept
    return d, a


def reference_mask(logits_bf16, rec, delta, accept, table, fed, eos):
    """The rule of include/p3v.h (p3v_guide_mask) on ONE row.  logits_bf16: uint16 [n] (bf16 bits); rec: the row's four record
    words {flags, n_states, state, reserved}; delta uint16 [256, 256] and accept uint8 [256]: the row's region; table: a
    VocabTable over at least n ids; fed: the token the step was fed, or None (the kernel's fed == NULL); eos: the EOS id.
    Returns (masked bits uint16 [n], the record's state afterwards)."""
    bits = np.array(logits_bf16, dtype=np.uint16)
    n = bits.shape[0]
    flags, n_states, state = int(rec[0]), int(rec[1]), int(rec[2])
    if not flags & ACTIVE:                                                      # 0.
        return bits, state
    delta = np.asarray(delta, dtype=np.uint16).reshape(256, 256)
    accept = np.asarray(accept, dtype=np.uint8).reshape(256)
    lens, mat = table.padded()
    lens, mat = lens[:n], mat[:n]
    good = 1 <= n_states <= MAX_STATES and (state == DONE or 1 <= state <= n_states)
    if good and state != DONE and fed is not None:                              # 1. (a record out of range is not written)
        f = int(fed)
        if f == int(eos):
            state = DONE
        elif 0 <= f < n and lens[f] > 0:
            state = int(_walk_all(delta, [state], lens[f:f + 1], mat[f:f + 1], n_states)[0])
    cur = state if good and 1 <= state <= n_states else DONE                    # 4. (a dead end counts as DONE as well)
    if cur == DONE:
        allowed = np.zeros(n, dtype=bool)
        eos_ok = True
    else:
        end = _walk_all(delta, np.full(n, cur), lens, mat, n_states)
        allowed = (lens > 0) & (end != 0)                                       # 2.
        eos_ok = bool(accept[cur])
    if 0 <= int(eos) < n:
        allowed[int(eos)] = eos_ok
    bits[~allowed] = NEG_INF                                                    # 3.
    return bits, state


# ---- a request's guide as one JSON-able dict (engine.guide_args, the fleet, the server)
FIELDS = ("regex", "choice")


def request_guide(d):
    """One request's {"regex": str} or {"choice": [str, ...]} -> its compiled guide, or None when it asks for none."""
    if d is None:
        return None
    if not isinstance(d, dict):
        raise ValueError(f"guide must be a mapping, got {type(d).__name__}")
    unknown = set(d) - set(FIELDS)
    if unknown:
        raise ValueError(f"unknown guide fields: {sorted(unknown)}")
    regex, choice = d.get("regex"), d.get("choice")
    if regex is not None and not isinstance(regex, str):
        raise ValueError(f"guided_regex must be a string, got {type(regex).__name__}")
    return compile_guide(regex, choice)
