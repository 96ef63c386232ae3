"""Host side of guided decoding: a regular expression (or a choice list, which is one) compiled to a byte-level DFA, the
vocabulary's byte table, the liveness check of a DFA against a vocabulary, and a plain NumPy restatement of the device rule.

The rule itself is written out in include/p3v.h above `p3v_guide_row_t`; the kernel in csrc/p3v_guide.hip implements it and
`reference_mask` here reproduces every output bit and every state.

A guide is a DFA over BYTES: states 1..S, state 0 dead, state 1 the start, `delta` uint16 [S + 1, 256], `accept` uint8 [S + 1].
A regular expression or a choice list holds S <= 255 states and travels to the device in the NARROW form (one table row of 256
entries per state); a JSON schema (`json_regex`, `compile_json`) may need more and then travels in the WIDE form, its table
compressed to the byte classes the guide distinguishes, bounded by (S + 1) * (C + 1) <= 65,536 entries (`region`, `record`).  It constrains the UTF-8 bytes of the whole output (full-match semantics): the concatenated byte strings of the
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
WIDE_MAX_ENTRIES = 65536              # P3V_GUIDE_WIDE_MAX_ENTRIES: (S + 1) * (C + 1) of a wide guide
DONE = -1                             # p3v_guide_row_t.state after EOS
ACTIVE = 1                            # P3V_GUIDE_ACTIVE (bit 0 of flags)
WIDE = 256                            # P3V_GUIDE_WIDE (bit 8 of flags): the record's `reserved` is then the class count C
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
        self._classes = None

    def classes(self):
        """The byte classes of the table -- its distinct columns: (cls uint8 [256], the class 0 .. C-1 of every byte; a
        representative byte of every class int64 [C])."""
        if self._classes is None:
            _, first, inv = np.unique(self.delta.T, axis=0, return_index=True, return_inverse=True)
            self._classes = (inv.reshape(-1).astype(np.uint8), first.astype(np.int64))
        return self._classes

    @property
    def n_classes(self):
        return len(self.classes()[1])

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
    def __init__(self, what="guided_regex"):
        self.what = what                                        # the option an error names
        self.eps = []                                           # state -> [states]
        self.edges = []                                         # state -> [(frozenset of bytes, state)]

    def new(self):
        self.eps.append([])
        self.edges.append([])
        if len(self.eps) > 200000:
            raise ValueError(f"{self.what}: the pattern expands to more than 200000 NFA states")
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
def _byte_classes(nfa):
    """The partition of 0..255 by the pattern's byte sets: (class of every byte int64 [256], the classes of every byte set)."""
    sets = list({bs for edges in nfa.edges for bs, _ in edges})
    if not sets:                                                # (the empty pattern: one class, no edge)
        return np.zeros(256, dtype=np.int64), {}
    member = np.zeros((len(sets), 256), dtype=bool)
    for i, bs in enumerate(sets):
        member[i, list(bs)] = True
    _, inv = np.unique(member.T, axis=0, return_inverse=True)
    inv = inv.reshape(-1).astype(np.int64)
    return inv, {bs: np.unique(inv[member[i]]).tolist() for i, bs in enumerate(sets)}


def _subset(nfa, start, final, wide=False):
    """-> (delta int64 [N, K] complete over N subsets and the K byte classes of the pattern, subset 0 = the start; accept bool
    [N]; the class of every byte int64 [256]).  Two bytes that no byte set of the pattern tells apart share a column."""
    byte_cls, classes_of = _byte_classes(nfa)
    K = int(byte_cls.max()) + 1
    s0 = nfa.closure([start])
    index, order, rows = {s0: 0}, [s0], []
    k = 0
    while k < len(order):
        cur = order[k]
        k += 1
        by_cls = {}
        for s in cur:
            for bs, t in nfa.edges[s]:
                for c in classes_of[bs]:
                    by_cls.setdefault(c, set()).add(t)
        row = np.full(K, -1, dtype=np.int64)
        memo = {}
        for c, ts in by_cls.items():
            key = frozenset(ts)
            if key not in memo:
                nxt = nfa.closure(key)
                if nxt not in index:
                    index[nxt] = len(order)
                    order.append(nxt)
                    if len(order) > _SUBSET_CAP:
                        holds = f"{WIDE_MAX_ENTRIES} table entries, (states + 1) * (byte classes + 1)" if wide else MAX_STATES
                        raise ValueError(f"{nfa.what}: more than {_SUBSET_CAP} states in the subset construction "
                                         f"(a guide holds at most {holds})")
                memo[key] = index[nxt]
            row[c] = memo[key]
        rows.append(row)
    delta = np.stack(rows)
    dead = len(order)                                           # one explicit dead state completes the table
    delta = np.concatenate([np.where(delta < 0, dead, delta), np.full((1, K), dead, dtype=np.int64)])
    accept = np.array([final in s for s in order] + [False])
    return delta, accept, byte_cls


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


def _finish(delta, accept, byte_cls, pattern, wide=False, what="guided_regex"):
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
        raise ValueError(f"{what}: {pattern!r} matches nothing")
    mdelta = mdelta[:, byte_cls]                                # back to one column per byte
    # renumber: 0 dead, 1 the start, the rest in breadth-first order from the start
    number, queue = {start: 1}, [start]
    for s in queue:
        for t in mdelta[s].tolist():
            if live[t] and t not in number:
                number[t] = len(number) + 1
                queue.append(t)
    S = len(number)
    if not wide and S > MAX_STATES:
        raise ValueError(f"guided_regex: {pattern!r} needs {S} states after minimisation; a guide holds at most {MAX_STATES}")
    num = np.zeros(n, dtype=np.int64)
    for s, k in number.items():
        num[s] = k
    out = np.zeros((S + 1, 256), dtype=np.uint16)
    acc = np.zeros(S + 1, dtype=np.uint8)
    out[1:] = num[mdelta[queue]]
    acc[1:] = maccept[queue]
    dfa = Dfa(out, acc, pattern)
    if wide and S > MAX_STATES and (S + 1) * (dfa.n_classes + 1) > WIDE_MAX_ENTRIES:
        C = dfa.n_classes
        raise ValueError(f"{what}: the guide needs {S} states and {C} byte classes after minimisation, ({S} + 1) * ({C} + 1) = "
                         f"{(S + 1) * (C + 1)} table entries; a guide holds at most {WIDE_MAX_ENTRIES}")
    return dfa


def _compile(pattern, wide=False, what="guided_regex"):
    ast = _Parser(pattern).parse()
    nfa = _Nfa(what)
    start, final = nfa.build(ast)
    return _finish(*_subset(nfa, start, final, wide), pattern, wide, what)


# ----------------------------------------------------------------------------- the host LRU cache of compiled guides
CACHE_SIZE = 64
_cache = OrderedDict()


def compile_regex(pattern):
    """The minimised, pruned DFA of `pattern` (full-match semantics over UTF-8 bytes); ValueError names an unsupported construct
    or the state count beyond 255.  Compiled guides are kept in a small LRU cache keyed by the pattern."""
    if not isinstance(pattern, str):
        raise ValueError(f"guided_regex must be a string, got {type(pattern).__name__}")
    return _cached(pattern, lambda: _compile(pattern))


def _cached(key, make):
    hit = _cache.get(key)
    if hit is not None:
        _cache.move_to_end(key)
        return hit
    dfa = make()
    _cache[key] = dfa
    while len(_cache) > CACHE_SIZE:
        _cache.popitem(last=False)
    return dfa


def compile_wide(pattern, what="guided_regex"):
    """`pattern` compiled under the WIDE bound: any number of states S whose class-compressed table fits, (S + 1) * (C + 1) <=
    65,536 entries with C the byte classes (the distinct columns) of the minimised table; up to 255 states always fit (the
    narrow form).  ValueError reports S, C and the bound otherwise.  Not cached: `compile_json` caches by schema."""
    if not isinstance(pattern, str):
        raise ValueError(f"a guide pattern must be a string, got {type(pattern).__name__}")
    return _compile(pattern, wide=True, what=what)


# ----------------------------------------------------------------------------- JSON schema -> pattern
_J_ANNOTATIONS = ("title", "description", "default", "examples", "$schema", "$id", "$defs", "definitions")
_J_REFUSED = {
    "pattern": "a string's own regular expression is not translated", "format": "formats are not translated",
    "minimum": "numeric bounds are not regular in a useful size", "maximum": "numeric bounds are not regular in a useful size",
    "exclusiveMinimum": "numeric bounds are not regular in a useful size",
    "exclusiveMaximum": "numeric bounds are not regular in a useful size", "multipleOf": "divisibility is not translated",
    "allOf": "an intersection of schemas is not translated", "not": "a complement is not translated",
    "if": "conditionals are not translated", "then": "conditionals are not translated", "else": "conditionals are not translated",
    "prefixItems": "tuple arrays are not translated (one `items` schema for every element)"}
_J_BY_TYPE = {"object": ("properties", "required", "additionalProperties"), "array": ("items", "minItems", "maxItems"),
              "string": ("minLength", "maxLength"), "integer": (), "number": (), "boolean": (), "null": ()}
_J_CHAR = r'(?:[^"\\\x00-\x1f]|\\(?:["\\/bfnrt]|u[0-9a-fA-F]{4}))'
_J_INTEGER = r"-?(?:0|[1-9][0-9]{0,17})"
_J_NUMBER = _J_INTEGER + r"(?:\.[0-9]{1,17})?(?:[eE][+-]?[0-9]{1,3})?"
_J_COLON, _J_COMMA = ": ?", ", ?"


def _j_fail(path, msg):
    raise ValueError(f"guided_json: {msg} (at {path or '#'})")


def _j_count(schema, key, path, default):
    if key not in schema:
        return default
    v = schema[key]
    if isinstance(v, bool) or not isinstance(v, int) or v < 0:
        _j_fail(path, f"{key} must be a non-negative integer, got {v!r}")
    return v


def _j_literal(v, path, key):
    import json
    if isinstance(v, float) and (v != v or v in (float("inf"), float("-inf"))):
        _j_fail(path, f"{key} holds {v!r}, which JSON cannot spell")
    if v is not None and not isinstance(v, (str, int, float, bool)):
        _j_fail(path, f"{key} takes scalars only (string, number, boolean, null), got {type(v).__name__}")
    return escape(json.dumps(v, ensure_ascii=False))


def _j_is(v, t):
    if t == "string":
        return isinstance(v, str)
    if t == "boolean":
        return isinstance(v, bool)
    if t == "null":
        return v is None
    if t == "integer":
        return isinstance(v, int) and not isinstance(v, bool)
    if t == "number":
        return isinstance(v, (int, float)) and not isinstance(v, bool)
    return False                                                # (enum / const hold scalars only)


def _j_alt(branches):
    seen = list(dict.fromkeys(branches))
    return seen[0] if len(seen) == 1 else "(?:" + "|".join(seen) + ")"


def _j_types(schema, path):
    t = schema.get("type")
    types = [t] if isinstance(t, str) else t
    if not isinstance(types, list) or not types or any(not isinstance(x, str) or x not in _J_BY_TYPE for x in types):
        _j_fail(path, f"type must be one of {sorted(_J_BY_TYPE)} or a non-empty list of them, got {t!r}")
    return types


def _j_node(schema, root, path, stack):
    if not isinstance(schema, dict):
        _j_fail(path, f"a schema must be an object, got {schema!r} (the schemas true and false are not translated)")
    for k in schema:
        if k in _J_REFUSED:
            _j_fail(path, f"the keyword {k!r} is not supported: {_J_REFUSED[k]}")
    keys = [k for k in schema if k not in _J_ANNOTATIONS]
    heads = [k for k in ("$ref", "anyOf", "oneOf", "enum", "const") if k in schema]
    if len(heads) > 1:
        _j_fail(path, f"{heads[0]!r} beside {heads[1]!r} is not translated: give one of them")
    head = heads[0] if heads else None
    if head in ("$ref", "anyOf", "oneOf"):                      # these stand alone (beside annotations)
        extra = [k for k in keys if k != head]
        if extra:
            _j_fail(path, f"the keyword {extra[0]!r} beside {head!r} is not translated (an intersection of schemas)")
    if head == "$ref":
        ref = schema["$ref"]
        m = _re.fullmatch(r"#/(\$defs|definitions)/([^/]+)", ref) if isinstance(ref, str) else None
        if m is None:
            _j_fail(path, f"$ref {ref!r} is not supported: only '#/$defs/NAME' and '#/definitions/NAME'")
        name = m.group(2).replace("~1", "/").replace("~0", "~")
        target = root.get(m.group(1)) if isinstance(root, dict) else None
        if not isinstance(target, dict) or name not in target:
            _j_fail(path, f"$ref {ref!r} points at nothing")
        if ref in stack:
            _j_fail(path, f"$ref {ref!r} is recursive ({' -> '.join(stack + (ref,))}): a recursive schema is not regular")
        return _j_node(target[name], root, ref, stack + (ref,))
    if head in ("anyOf", "oneOf"):
        subs = schema[head]
        if not isinstance(subs, list) or not subs:
            _j_fail(path, f"{head} must be a non-empty list of schemas")
        return _j_alt([_j_node(sub, root, f"{path}/{head}/{i}", stack) for i, sub in enumerate(subs)])
    if head in ("enum", "const"):
        extra = [k for k in keys if k not in (head, "type")]
        if extra:
            _j_fail(path, f"the keyword {extra[0]!r} beside {head!r} is not translated")
        values = [schema["const"]] if head == "const" else schema["enum"]
        if not isinstance(values, list) or not values:
            _j_fail(path, "enum must be a non-empty list of scalars")
        lits = [(v, _j_literal(v, path, head)) for v in values]
        if "type" in schema:                                    # both hold: the values of the enum that have the type
            types = _j_types(schema, path)
            lits = [(v, lit) for v, lit in lits if any(_j_is(v, t) for t in types)]
            if not lits:
                _j_fail(path, f"no value of {head} has the type {schema['type']!r}: the schema matches nothing")
        return _j_alt([lit for _, lit in lits])
    if "type" not in schema:
        _j_fail(path, "a schema needs one of type, enum, const, anyOf, oneOf or $ref (free-form JSON is not regular)")
    types = _j_types(schema, path)
    known = {"type"} | {k for t in types for k in _J_BY_TYPE[t]}
    for k in keys:
        if k not in known:
            where = [t for t, ks in _J_BY_TYPE.items() if k in ks]
            _j_fail(path, f"the keyword {k!r} does not apply to type {schema['type']!r}" if where else f"unknown keyword {k!r}")
    return _j_alt([_J_OF_TYPE[t](schema, root, path, stack) for t in types])


def _j_object(schema, root, path, stack):
    import json
    if schema.get("additionalProperties", False) is not False:
        _j_fail(path, "additionalProperties other than false is not supported: an object holds its declared properties only")
    props = schema.get("properties")
    if not isinstance(props, dict):
        _j_fail(path, "an object needs properties (a free-form object is not regular)")
    required = schema.get("required", [])
    if not isinstance(required, list) or any(not isinstance(r, str) for r in required):
        _j_fail(path, "required must be a list of property names")
    for r in required:
        if r not in props:
            _j_fail(path, f"required names {r!r}, which is not among the properties: the schema matches nothing")
    members = [(escape(json.dumps(k, ensure_ascii=False)) + _J_COLON + _j_node(v, root, f"{path}/properties/{k}", stack), k in required)
               for k, v in props.items()]
    # declared order; the branches differ in WHICH property comes first (no required one may lie before it), the properties
    # behind it follow with their commas, the optional ones in (?: )?
    branches = []
    for i, (first, _) in enumerate(members):
        rest = "".join(_J_COMMA + m if req else "(?:" + _J_COMMA + m + ")?" for m, req in members[i + 1:])
        branches.append(first + rest)
        if members[i][1]:
            break
    else:
        branches.append("")                                     # no required property: {} matches
    body = branches[0] if len(branches) == 1 else "(?:" + "|".join(branches) + ")"
    return r"\{" + body + r"\}"


def _j_array(schema, root, path, stack):
    if "items" not in schema:
        _j_fail(path, "an array needs items (a free-form array is not regular)")
    lo, hi = _j_count(schema, "minItems", path, 0), _j_count(schema, "maxItems", path, None)
    if hi is not None and hi < lo:
        _j_fail(path, f"minItems {lo} > maxItems {hi}: the schema matches nothing")
    if hi == 0:
        return r"\[\]"
    item = _j_node(schema["items"], root, f"{path}/items", stack)
    more = "(?:" + _J_COMMA + item + ")" + ("{%d,}" % max(lo - 1, 0) if hi is None else "{%d,%d}" % (max(lo - 1, 0), hi - 1))
    return r"\[" + (item + more if lo >= 1 else "(?:" + item + more + ")?") + r"\]"


def _j_string(schema, root, path, stack):
    lo, hi = _j_count(schema, "minLength", path, 0), _j_count(schema, "maxLength", path, None)
    if hi is not None and hi < lo:
        _j_fail(path, f"minLength {lo} > maxLength {hi}: the schema matches nothing")
    rep = ("*" if lo == 0 else "{%d,}" % lo) if hi is None else "{%d,%d}" % (lo, hi)
    return '"' + _J_CHAR + rep + '"'


_J_OF_TYPE = {"object": _j_object, "array": _j_array, "string": _j_string, "integer": lambda *a: _J_INTEGER,
              "number": lambda *a: _J_NUMBER, "boolean": lambda *a: "(?:true|false)", "null": lambda *a: "null"}


def _j_schema(schema):
    """A dict, or a JSON text of one -> (the dict, its cache key: the JSON text in DECLARED key order)."""
    import json
    if isinstance(schema, (str, bytes)):
        try:
            schema = json.loads(schema)
        except ValueError as e:
            raise ValueError(f"guided_json: the schema is not valid JSON: {e}") from None
    if not isinstance(schema, dict):
        raise ValueError(f"guided_json must be a JSON schema (an object or its JSON text), got {type(schema).__name__}")
    try:
        return schema, json.dumps(schema, separators=(",", ":"), allow_nan=False)
    except (TypeError, ValueError) as e:
        raise ValueError(f"guided_json: the schema is not JSON: {e}") from None


def json_regex(schema):
    """A JSON schema (a dict or its JSON text) as a pattern of this module's regex subset: the JSON texts of the instances that
    satisfy it.  Every keyword is translated, ignored as an annotation, or refused with a ValueError that names it:
      type       object, array, string, integer, number, boolean, null, or a list of them (an alternation);
      object     `properties` in DECLARED order, `required` (the others are optional and keep their place in that order);
                 `additionalProperties` absent or false; true or a schema is refused, as is an object without `properties`;
      array      `items` (one schema), `minItems`, `maxItems`; `prefixItems` and an array without `items` are refused;
      string     any code point except `"`, `\\` and those below 0x20, and the escapes \\" \\\\ \\/ \\b \\f \\n \\r \\t \\uXXXX;
                 `minLength` / `maxLength`; `pattern` and `format` are refused;
      integer    -?(0|[1-9][0-9]{0,17});  number: that plus an optional fraction of 1..17 digits and an exponent of 1..3 digits;
                 minimum, maximum, exclusiveMinimum, exclusiveMaximum and multipleOf are refused;
      enum/const scalars only, each as json.dumps(v, ensure_ascii=False); beside `type`, the values that have the type;
      anyOf/oneOf  an alternation; allOf, not, if / then / else are refused;
      $ref       to #/$defs/NAME or #/definitions/NAME, inlined; a cycle raises and names the reference;
      ignored    title, description, default, examples, $schema, $id, $defs, definitions.
    Whitespace: ONE optional space after ':' and after ',' and nowhere else, so json.dumps(x) and json.dumps(x, separators=
    (",", ":")) of a valid instance both match -- in declared key order.
    Departures from the JSON Schema specification: the key order is fixed (declared order) and no key may repeat; other keys are
    never allowed (`additionalProperties` defaults to false, not true); `oneOf` is `anyOf` (an instance that satisfies two
    branches matches); `minLength` / `maxLength` count one per character or escape, so a surrogate pair written as two \\uXXXX
    escapes counts two; integers hold at most 18 digits, fractions 17, exponents 3, and `1.0` or `1e2` is not an integer;
    a keyword of another type (`minLength` beside type integer), `enum` / `const` beside anything but `type`, and anyOf / oneOf /
    $ref beside other keywords are refused instead of being combined; the schemas `true`, `false` and `{}` are refused."""
    schema, _ = _j_schema(schema)
    return _j_node(schema, schema, "", ())


def compile_json(schema):
    """The guide of a JSON schema (a dict or its JSON text): `json_regex` through the same compiler under the wide bound
    (`compile_wide`).  ValueError names a refused keyword, or the state count, class count and bound of a guide that does not
    fit.  Compiled guides share the LRU cache of the patterns, keyed by the schema's JSON text -- in declared key order, NOT
    sort_keys: the order of `properties` is part of the meaning here."""
    schema, key = _j_schema(schema)
    return _cached(("json", key), lambda: compile_wide(_j_node(schema, schema, "", ()), what="guided_json"))


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


def exclusive(regex=None, choice=None, schema=None):
    """At most one kind of guide per prompt: two at once raise, naming them."""
    given = [name for name, v in (("guided_regex", regex), ("guided_choice", choice), ("guided_json", schema)) if v is not None]
    if len(given) > 1:
        raise ValueError(f"{', '.join(given[:-1])} and {given[-1]} exclude each other: give one per prompt")


def compile_guide(regex=None, choice=None, schema=None):
    """One request's guide: None when it asks for none; two kinds at once raise."""
    exclusive(regex, choice, schema)
    if regex is not None:
        return compile_regex(regex)
    if choice is not None:
        return compile_choice(choice)
    if schema is not None:
        return compile_json(schema)
    return None


def per_prompt(B, regex=None, choice=None, schema=None):
    """The public arguments -- each one value for every prompt, or a list of one value / None per prompt -- as B compiled
    guides / None, or None when no prompt has one.  (A choice list is a list of strings: a per-prompt list of choices is a
    list of lists / None.  A schema is a dict or its JSON text: a list is one schema / None per prompt.)"""
    if isinstance(schema, (list, tuple)):
        if len(schema) != B:
            raise ValueError(f"guided_json: {len(schema)} values for {B} prompts")
        sc = list(schema)
    else:
        sc = [schema] * B
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
    out = [compile_guide(r, c, s) for r, c, s in zip(rx, ch, sc)]
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
def is_wide(dfa, wide=None):
    """Does this guide travel in the wide form?  Above 255 states it must; `wide=True` forces a smaller one into it."""
    return dfa.n_states > MAX_STATES if wide is None else bool(wide) or dfa.n_states > MAX_STATES


def wide_pitch(n_states, n_classes):
    """The row pitch of a wide table (include/p3v.h): C + 1 columns, padded to an odd count where rows 0..S still fit."""
    odd = (n_classes + 1) | 1
    return odd if (n_states + 1) * odd <= WIDE_MAX_ENTRIES else n_classes + 1


def record(dfa, state=1, wide=None):
    """One row's p3v_guide_row_t words: an inactive row for None; the narrow form up to 255 states, the wide form (the flag,
    and the class count in `reserved`) above -- or where `wide` forces it."""
    if dfa is None:
        return [0, 0, 0, 0]
    if is_wide(dfa, wide):
        return [ACTIVE | WIDE, dfa.n_states, int(state), dfa.n_classes]
    return [ACTIVE, dfa.n_states, int(state), 0]


def region(dfa, wide=None):
    """A guide as one row's table region, (delta uint16 [256, 256], accept uint8 [256]), zero beyond what it fills.  Narrow (up
    to 255 states): the dense table and the accept flags.  Wide (above, or forced): `accept` holds the class of every byte and
    `delta`, read flat, the table [S + 1, pitch] -- column 0 the accept flag, column 1 + c the successor on class c."""
    d = np.zeros((256, 256), dtype=np.uint16)
    a = np.zeros(256, dtype=np.uint8)
    S = dfa.n_states
    if not is_wide(dfa, wide):
        d[:S + 1] = dfa.delta
        a[:S + 1] = dfa.accept
        return d, a
    cls, rep = dfa.classes()
    C = len(rep)
    if (S + 1) * (C + 1) > WIDE_MAX_ENTRIES:
        raise ValueError(f"a guide of {S} states and {C} byte classes needs ({S} + 1) * ({C} + 1) = {(S + 1) * (C + 1)} table "
                         f"entries; a guide holds at most {WIDE_MAX_ENTRIES}")
    pitch = wide_pitch(S, C)
    table = d.reshape(-1)[:(S + 1) * pitch].reshape(S + 1, pitch)
    table[:, 0] = dfa.accept
    table[:, 1:C + 1] = dfa.delta[:, rep]
    a[:] = cls
    return d, a


def region_rows(dfa, wide=None):
    """How many of the 256 rows of `region(dfa)[0]` the guide fills (the rest is zero and never read)."""
    S = dfa.n_states
    return -(-(S + 1) * wide_pitch(S, dfa.n_classes) // 256) if is_wide(dfa, wide) else S + 1


def _dense(n_states, n_classes, region_delta, region_cls):
    """A wide row's region read back as the rule's walk sees it: (delta int64 [S + 1, 256], accept uint8 [S + 1])."""
    pitch = wide_pitch(n_states, n_classes)
    table = np.asarray(region_delta, dtype=np.uint16).reshape(-1)[:(n_states + 1) * pitch].reshape(n_states + 1, pitch).astype(np.int64)
    table[table > n_states] = 0                                                 # an entry above S counts as 0, in every column
    cls = np.asarray(region_cls, dtype=np.uint8).reshape(256).astype(np.int64)
    delta = np.where(cls[None, :] < n_classes, table[:, 1 + np.minimum(cls, n_classes - 1)], 0)   # a class outside 0..C-1: dead
    return delta, (table[:, 0] != 0).astype(np.uint8)


def reference_mask(logits_bf16, rec, delta, accept, table, fed, eos):
    """The rule of include/p3v.h (p3v_guide_mask) on ONE row.  logits_bf16: uint16 [n] (bf16 bits); rec: the row's four record
    words {flags, n_states, state, reserved}; delta uint16 [256, 256] and accept uint8 [256]: the row's region; table: a
    VocabTable over at least n ids; fed: the token the step was fed, or None (the kernel's fed == NULL); eos: the EOS id.
    A record with the WIDE flag reads the same region as the wide form (cls in `accept`, the class-compressed table in `delta`,
    C in the record's fourth word); the rule is the same from there on.
    Returns (masked bits uint16 [n], the record's state afterwards)."""
    bits = np.array(logits_bf16, dtype=np.uint16)
    n = bits.shape[0]
    flags, n_states, state = int(rec[0]), int(rec[1]), int(rec[2])
    if not flags & ACTIVE:                                                      # 0.
        return bits, state
    lens, mat = table.padded()
    lens, mat = lens[:n], mat[:n]
    good = n_states >= 1 and (state == DONE or 1 <= state <= n_states)
    if flags & WIDE:
        n_classes = int(rec[3])
        good = good and 1 <= n_classes <= 256 and (n_states + 1) * (n_classes + 1) <= WIDE_MAX_ENTRIES
        if good:
            delta, accept = _dense(n_states, n_classes, delta, accept)
    else:
        good = good and n_states <= MAX_STATES
        delta = np.asarray(delta, dtype=np.uint16).reshape(256, 256)
        accept = np.asarray(accept, dtype=np.uint8).reshape(256)
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
FIELDS = ("regex", "choice", "schema")


def request_guide(d):
    """One request's {"regex": str}, {"choice": [str, ...]} or {"schema": a JSON schema (a dict or its JSON text)} -> its compiled
    guide, or None when it asks for none."""
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
    return compile_guide(regex, choice, d.get("schema"))
