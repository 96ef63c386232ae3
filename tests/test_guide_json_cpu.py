"""guided_json on the host: the schema translator (guide.json_regex / compile_json) against an oracle written HERE -- json.loads
plus a small recursive validator of the subset --, the refusals, the limits, the wide form of a guide's region and record against
the narrow one, and the option through request record, engine carrier and server fields.  No GPU."""
import json
import random
import re
import string

import numpy as np
import pytest

from phi_3_vision_mlx_amd import guide, penalties

# ----------------------------------------------------------------------------- the oracle
TYPES = {"object": dict, "array": list, "string": str, "boolean": bool, "null": type(None)}


def _has_type(x, t):
    if t == "integer":
        return isinstance(x, int) and not isinstance(x, bool)
    if t == "number":
        return isinstance(x, (int, float)) and not isinstance(x, bool)
    return isinstance(x, TYPES[t])


def validate(schema, x, root=None):
    """Does the parsed instance x satisfy the schema (the subset the translator takes; no other key is ever allowed)?"""
    root = schema if root is None else root
    if "$ref" in schema:
        kind, name = schema["$ref"].split("/")[1:]
        return validate(root[kind][name], x, root)
    for k in ("anyOf", "oneOf"):
        if k in schema:
            return any(validate(s, x, root) for s in schema[k])
    if "const" in schema or "enum" in schema:
        vals = [schema["const"]] if "const" in schema else schema["enum"]
        if not any(type(v) is type(x) and v == x for v in vals):
            return False
        if "type" not in schema:
            return True
    types = schema["type"] if isinstance(schema["type"], list) else [schema["type"]]
    ok = [t for t in types if _has_type(x, t)]
    if not ok:
        return False
    if "enum" in schema or "const" in schema:
        return True
    if isinstance(x, dict):
        props = schema["properties"]
        if any(k not in props for k in x) or any(r not in x for r in schema.get("required", [])):
            return False
        return all(validate(props[k], v, root) for k, v in x.items())
    if isinstance(x, list):
        if not schema.get("minItems", 0) <= len(x) <= schema.get("maxItems", 10 ** 9):
            return False
        return all(validate(schema["items"], v, root) for v in x)
    if isinstance(x, str):
        return schema.get("minLength", 0) <= len(x) <= schema.get("maxLength", 10 ** 9)
    return True


def in_declared_order(schema, x, root=None):
    """The translator fixes the key order: an instance whose keys come in another order is not in the language."""
    root = schema if root is None else root
    if "$ref" in schema:
        kind, name = schema["$ref"].split("/")[1:]
        return in_declared_order(root[kind][name], x, root)
    for k in ("anyOf", "oneOf"):
        if k in schema:
            return any(validate(s, x, root) and in_declared_order(s, x, root) for s in schema[k])
    if isinstance(x, dict) and "properties" in schema:
        order = [k for k in schema["properties"] if k in x]
        return list(x) == order and all(in_declared_order(schema["properties"][k], v, root) for k, v in x.items())
    if isinstance(x, list) and "items" in schema:
        return all(in_declared_order(schema["items"], v, root) for v in x)
    return True


# ----------------------------------------------------------------------------- schemas covering every keyword, and their instances
PERSON = {"$schema": "https://json-schema.org/draft/2020-12/schema", "$id": "person", "title": "Person", "type": "object",
          "properties": {"name": {"type": "string", "minLength": 1, "maxLength": 5, "description": "given name"},
                         "age": {"type": "integer", "default": 0},
                         "email": {"type": ["string", "null"], "examples": ["a@b"]},
                         "score": {"type": "number"}},
          "required": ["name", "age"], "additionalProperties": False}
TAGS = {"type": "object",
        "properties": {"tags": {"type": "array", "items": {"$ref": "#/$defs/tag"}, "minItems": 1, "maxItems": 3},
                       "active": {"type": "boolean"}, "kind": {"const": "tool"},
                       "level": {"enum": ["low", "hi\"gh", 3, 2.5, True, None, "é"]},
                       "n": {"type": "integer", "enum": [1, "x", 7]}},
        "$defs": {"tag": {"type": "string", "maxLength": 2}}}
CALL = {"oneOf": [{"type": "object", "properties": {"tool": {"const": "add"}, "args": {"$ref": "#/definitions/pair"}}, "required": ["tool", "args"]},
                  {"type": "object", "properties": {"tool": {"enum": ["now", "quit"]}}, "required": ["tool"]},
                  {"type": "null"}],
        "definitions": {"pair": {"type": "array", "items": {"anyOf": [{"type": "integer"}, {"type": "boolean"}]}, "minItems": 2, "maxItems": 2}}}
LIST = {"type": "array", "maxItems": 2,
        "items": {"type": "object", "properties": {"x": {"type": "number"}, "e": {"type": "object", "properties": {}}, "s": {"type": "string"}}}}
SCHEMAS = {"person": PERSON, "tags": TAGS, "call": CALL, "list": LIST}
CHARS = ["a", "Z", " ", "é", "€", "\U0001F600", '"', "\\", "/", "\n", "\t", "\b", "\x01", "{", ","]


def generate(schema, rng, root=None, edge=None):
    """A random instance of the schema; edge "min" / "max" pushes arrays, strings and optional properties to their ends."""
    root = schema if root is None else root
    if "$ref" in schema:
        kind, name = schema["$ref"].split("/")[1:]
        return generate(root[kind][name], rng, root, edge)
    for k in ("anyOf", "oneOf"):
        if k in schema:
            return generate(rng.choice(schema[k]), rng, root, edge)
    if "const" in schema:
        return schema["const"]
    if "enum" in schema:
        vals = [v for v in schema["enum"] if "type" not in schema or _has_type(v, schema["type"])]
        return rng.choice(vals)
    t = rng.choice(schema["type"]) if isinstance(schema["type"], list) else schema["type"]
    if t == "object":
        req = schema.get("required", [])
        keep = {"min": lambda: False, "max": lambda: True}.get(edge, lambda: rng.random() < 0.5)
        return {k: generate(v, rng, root, edge) for k, v in schema["properties"].items() if k in req or keep()}
    if t == "array":
        lo, hi = schema.get("minItems", 0), schema.get("maxItems", schema.get("minItems", 0) + 3)
        k = {"min": lo, "max": hi}.get(edge, rng.randint(lo, hi))
        return [generate(schema["items"], rng, root, edge) for _ in range(k)]
    if t == "string":
        lo, hi = schema.get("minLength", 0), schema.get("maxLength", schema.get("minLength", 0) + 6)
        k = {"min": lo, "max": hi}.get(edge, rng.randint(lo, hi))
        return "".join(rng.choice(CHARS) for _ in range(k))
    if t == "integer":
        return rng.choice([0, -0, -1, 7, -10 ** 17, 10 ** 18 - 1, rng.randint(-999, 999)])
    if t == "number":
        return rng.choice([0, -3, 0.5, -2.25, 1e-7, 1.5e+300, 123456.789, rng.randint(-99, 99)])
    return {"boolean": rng.choice([True, False]), "null": None}[t]


def spellings(x):
    """json.dumps in both separator styles (non-ASCII characters as themselves, which is how enum / const literals are spelled; the
    characters JSON must escape -- quote, backslash, control characters -- are escaped in either)"""
    return [json.dumps(x, ensure_ascii=False), json.dumps(x, separators=(",", ":"), ensure_ascii=False)]


_INSTANCES = {}


def instances(name):
    if name not in _INSTANCES:
        rng = random.Random(sum(map(ord, name)))
        schema = SCHEMAS[name]
        out = [generate(schema, rng, edge="min"), generate(schema, rng, edge="max")] + [generate(schema, rng) for _ in range(60)]
        assert all(validate(schema, x) for x in out)
        _INSTANCES[name] = out
    return _INSTANCES[name]


@pytest.mark.parametrize("name", sorted(SCHEMAS))
def test_valid_instances_match_in_both_separator_styles(name):
    schema = SCHEMAS[name]
    dfa = guide.compile_json(schema)
    pattern = guide.json_regex(schema)
    oracle = re.compile(pattern, re.ASCII)
    texts = set()
    for x in instances(name):
        for text in spellings(x):
            assert dfa.matches(text), text
            assert oracle.fullmatch(text), text
            assert validate(schema, json.loads(text))
            texts.add(text)
    assert len(texts) > 20
    assert guide.compile_json(json.dumps(schema)) is dfa                         # a JSON text of the schema: the same cached guide


def test_instances_cover_the_corners():
    seen = [x for x in instances("person")]
    assert any("email" not in x for x in seen) and any("email" in x for x in seen) and any(x.get("email", 0) is None for x in seen)
    assert any(x["age"] == 0 for x in seen) and any(x["age"] < 0 for x in seen)
    assert any(any(ord(c) > 127 for c in x["name"]) for x in seen) and any('"' in x["name"] or "\\" in x["name"] for x in seen)
    tags = [x["tags"] for x in instances("tags") if "tags" in x]
    assert {len(t) for t in tags} >= {1, 3}


@pytest.mark.parametrize("name", sorted(SCHEMAS))
def test_accepted_strings_are_valid(name):
    """random accepting walks over the DFA: every accepted byte string is JSON and satisfies the schema"""
    schema = SCHEMAS[name]
    dfa = guide.compile_json(schema)
    rng = np.random.default_rng(7)
    # the shortest distance of every state to an accepting one, to steer a walk home once it is long enough
    S = dfa.n_states
    dist = np.where(dfa.accept[:S + 1] != 0, 0, 10 ** 9)
    for _ in range(S + 1):
        nxt = dist[dfa.delta].min(axis=1) + 1
        nxt[0] = 10 ** 9
        dist = np.minimum(dist, nxt)
    found = set()
    for k in range(300):
        s, out = 1, bytearray()
        budget = int(rng.integers(0, 60))
        while True:
            if dfa.accept[s] and (len(out) >= budget or rng.random() < 0.3):
                break
            succ = dfa.delta[s]
            live = np.flatnonzero(succ)
            if not len(live):                                    # (an accepting state without a way on)
                break
            if len(out) >= budget:
                live = live[dist[succ[live]] < dist[s]] if not dfa.accept[s] else live
            b = int(rng.choice(live))
            out.append(b)
            s = int(succ[b])
        text = bytes(out).decode("utf-8")                        # (a guide only ever spells well-formed UTF-8)
        x = json.loads(text)
        # the translator counts a surrogate pair written as two \uXXXX escapes as two characters: keep those out of the length check
        if not re.search(r"\\u[dD][89abAB]", text):
            assert validate(schema, x), text
        assert in_declared_order(schema, x), text
        found.add(text)
    assert len(found) > 10


def _broken(text, rng, k):
    out = set()
    alphabet = '{}[]",: 0-9aetrufnl\\.E+xé'
    for _ in range(k):
        i = rng.randrange(len(text))
        out.add(text[:i] + text[i + 1:])
        out.add(text[:i] + rng.choice(alphabet) + text[i + 1:])
    return out


@pytest.mark.parametrize("name", sorted(SCHEMAS))
def test_broken_instances_do_not_match(name):
    schema = SCHEMAS[name]
    dfa = guide.compile_json(schema)
    oracle = re.compile(guide.json_regex(schema), re.ASCII)
    rng = random.Random(11)
    tried = agreed = 0
    for x in instances(name):
        for text in spellings(x)[:2]:
            for bad in _broken(text, rng, 8):
                assert dfa.matches(bad) == bool(oracle.fullmatch(bad)), bad     # the compiler against `re`, on every string
                agreed += 1
                try:
                    y = json.loads(bad)
                    wrong = not validate(schema, y) or not in_declared_order(schema, y)
                except ValueError:
                    wrong = True
                if wrong:
                    tried += 1
                    assert not dfa.matches(bad), bad
    assert tried >= 300, tried


# ----------------------------------------------------------------------------- refusals
OBJ = {"type": "object", "properties": {"a": {"type": "integer"}}}


@pytest.mark.parametrize("schema, word", [
    ({"type": "string", "pattern": "a+"}, "pattern"), ({"type": "string", "format": "date"}, "format"),
    ({"type": "integer", "minimum": 0}, "minimum"), ({"type": "integer", "maximum": 9}, "maximum"),
    ({"type": "number", "exclusiveMinimum": 0}, "exclusiveMinimum"), ({"type": "number", "exclusiveMaximum": 1}, "exclusiveMaximum"),
    ({"type": "integer", "multipleOf": 2}, "multipleOf"), ({"allOf": [OBJ]}, "allOf"), ({"not": OBJ}, "not"),
    ({"if": OBJ, "then": OBJ, "else": OBJ}, "'if'"), ({"type": "object", "then": OBJ}, "then"), ({"type": "object", "else": OBJ}, "else"),
    ({"type": "array", "prefixItems": [OBJ]}, "prefixItems"), ({"type": "array"}, "items"), ({"type": "object"}, "properties"),
    (dict(OBJ, additionalProperties=True), "additionalProperties"), (dict(OBJ, additionalProperties={"type": "string"}), "additionalProperties"),
    (dict(OBJ, patternProperties={}), "patternProperties"), (dict(OBJ, frobnicate=1), "frobnicate"),
    ({"type": "array", "items": OBJ, "uniqueItems": True}, "uniqueItems"), ({"type": "integer", "minLength": 2}, "minLength"),
    ({"enum": [[1]]}, "enum"), ({"const": {"a": 1}}, "const"), ({"enum": []}, "enum"), ({"type": "str"}, "type"), ({}, "type"),
    ({"$ref": "#/$defs/a", "$defs": {"a": {"$ref": "#/$defs/b"}, "b": {"type": "array", "items": {"$ref": "#/$defs/a"}}}}, "#/\\$defs/a"),
    ({"$ref": "other.json#/x"}, "\\$ref"), ({"$ref": "#/$defs/nope", "$defs": {}}, "nope"),
    ({"type": "array", "items": OBJ, "minItems": 3, "maxItems": 2}, "minItems"), (dict(OBJ, required=["b"]), "required"),
    ({"type": "integer", "enum": ["x"]}, "enum"), ({"anyOf": [OBJ], "type": "object"}, "anyOf"),
    ({"type": "string", "maxLength": None}, "maxLength"), ({"type": "string", "minLength": None}, "minLength"),
    ({"type": "array", "items": OBJ, "maxItems": None}, "maxItems"), ({"type": "array", "items": OBJ, "minItems": 1.5}, "minItems"),
])
def test_refused_keywords_raise_and_name_themselves(schema, word):
    with pytest.raises(ValueError, match=word):
        guide.json_regex(schema)
    with pytest.raises(ValueError, match=word):
        guide.compile_json(json.dumps(schema))


def test_a_schema_too_large_to_compile_names_its_own_option_and_bound():
    props = {f"p{i}": {"type": "string", "maxLength": 40} for i in range(10)}
    with pytest.raises(ValueError) as e:
        guide.compile_json({"type": "object", "properties": props})
    assert str(e.value).startswith("guided_json:") and "NFA states" in str(e.value) and "guided_regex" not in str(e.value)
    with pytest.raises(ValueError) as e:                         # (no schema of the subset is this non-deterministic: the pattern path)
        guide.compile_wide("(a|b)*a(a|b){15}", what="guided_json")
    assert str(e.value).startswith("guided_json:") and "65536 table entries" in str(e.value) and "255" not in str(e.value), str(e.value)
    with pytest.raises(ValueError, match="guided_regex: more than 20000 states in the subset construction \\(a guide holds at most 255\\)"):
        guide.compile_regex("(a|b)*a(a|b){15}")


def test_bad_schema_values():
    for bad in (3, None, [OBJ], "not json", "[1]", True):
        with pytest.raises(ValueError, match="guided_json"):
            guide.compile_json(bad)


def test_property_order_is_part_of_the_cache_key():
    ab = {"type": "object", "properties": {"a": {"type": "null"}, "b": {"type": "null"}}, "required": ["a", "b"]}
    ba = {"type": "object", "properties": {"b": {"type": "null"}, "a": {"type": "null"}}, "required": ["a", "b"]}
    assert guide.compile_json(ab).matches('{"a":null,"b":null}') and not guide.compile_json(ab).matches('{"b":null,"a":null}')
    assert guide.compile_json(ba).matches('{"b":null,"a":null}') and not guide.compile_json(ba).matches('{"a":null,"b":null}')
    for i in range(guide.CACHE_SIZE + 5):
        guide.compile_json({"const": i})
    assert len(guide._cache) <= guide.CACHE_SIZE


# ----------------------------------------------------------------------------- the limits and the two forms
BOOK = {"type": "object", "properties": {"title": {"type": "string", "maxLength": 32}, "year": {"type": "integer"}}, "required": ["title", "year"]}
# 83 strings of 13 characters, each with a first character of its own: 900 states x 85 byte classes, over the entry bound
HUGE = {"enum": [c + ("%02d" % i) * 6 for i, c in enumerate(string.ascii_letters + string.digits + "!#$%&()*+-.:;<=>?@^_~")]}


def test_the_limits():
    dfa = guide.compile_json(BOOK)
    S, C = dfa.n_states, dfa.n_classes
    assert S > 255 and S == len(dfa.delta) - 1 and 20 < C < 64, (S, C)
    assert C == len(np.unique(dfa.delta.T, axis=0))                              # the distinct columns of the minimised table
    assert guide.record(dfa) == [guide.ACTIVE | guide.WIDE, S, 1, C] and guide.WIDE == 256 and guide.WIDE_MAX_ENTRIES == 65536
    assert guide.record(dfa, 7)[2] == 7 and guide.record(None) == [0, 0, 0, 0]
    small = guide.compile_json(PERSON)
    assert small.n_states <= 255 and guide.record(small) == [guide.ACTIVE, small.n_states, 1, 0]       # a small schema stays narrow
    with pytest.raises(ValueError) as e:
        guide.compile_json(HUGE)
    m = re.search(r"needs (\d+) states and (\d+) byte classes.*= (\d+) table entries.*at most 65536", str(e.value))
    assert m, str(e.value)
    s, c, total = map(int, m.groups())
    assert (s + 1) * (c + 1) == total > 65536
    with pytest.raises(ValueError, match="301 states"):
        guide.compile_regex("a{300}")
    with pytest.raises(ValueError, match="at most 255"):
        guide.compile_choice(["a" * 300])
    assert guide.compile_wide("a{300}").n_states == 301


def _vocab_table():
    rng = np.random.default_rng(3)
    alphabet = np.frombuffer('{}[]":, 0123456789abtrueflsn\\ué-.'.encode(), dtype=np.uint8)
    strings = [b""] + [bytes([b]) for b in range(256)]
    strings += [bytes(rng.choice(alphabet, int(rng.integers(2, 6))).tolist()) for _ in range(700)]
    strings += [b'{"title":"', b'","year":', b'", "year": ', b"", b"true", b"null", b'{"name": "']
    return guide.VocabTable(strings), 0                          # id 0: the EOS, no bytes


@pytest.mark.parametrize("name", ["book", "person", "regex", "one-state"])
def test_wide_and_narrow_forms_agree_on_every_state(name):
    """region / record round-trip through reference_mask; a guide of S <= 255 forced into the wide form gives, state by state,
    the masks and successor states of its narrow form (the restatement of the rule against itself)"""
    dfa = {"book": lambda: guide.compile_json(BOOK), "person": lambda: guide.compile_json(PERSON),
           "regex": lambda: guide.compile_regex("(ab|b\\.a)+[0-9]{1,3}é?"), "one-state": lambda: guide.compile_regex("[ab]*")}[name]()
    table, eos = _vocab_table()
    S, C = dfa.n_states, dfa.n_classes
    wd, wa = guide.region(dfa, wide=True)
    assert wd.shape == (256, 256) and wd.dtype == np.uint16 and wa.shape == (256,) and wa.dtype == np.uint8
    pitch = guide.wide_pitch(S, C)
    assert pitch in (C + 1, C + 2) and (pitch % 2 == 1 or (S + 1) * (pitch + 1) > 65536) and (S + 1) * pitch <= 65536
    flat = wd.reshape(-1)
    assert not flat[(S + 1) * pitch:].any() and int(wa.max()) == C - 1
    assert guide.region_rows(dfa, wide=True) * 256 >= (S + 1) * pitch > (guide.region_rows(dfa, wide=True) - 1) * 256
    tab = flat[:(S + 1) * pitch].reshape(S + 1, pitch)
    assert np.array_equal(tab[:, 0], dfa.accept) and np.array_equal(tab[:, 1 + wa.astype(np.int64)], dfa.delta)    # lossless
    narrow = S <= 255
    if narrow:
        nd, na = guide.region(dfa)
        assert np.array_equal(nd[:S + 1], dfa.delta) and np.array_equal(na[:S + 1], dfa.accept)
    else:
        assert all(np.array_equal(a, b) for a, b in zip(guide.region(dfa), (wd, wa)))            # above 255: wide without asking
    rng = np.random.default_rng(S)
    bits = penalties.f32_to_bf16_bits(rng.normal(0, 4, table.n).astype(np.float32))
    lens, mat = table.padded()
    states = range(1, S + 1) if S <= 300 else [1, 2, 255, 256, 257, S - 1, S] + rng.integers(1, S + 1, 40).tolist()
    for s in states:
        fed = int(rng.integers(0, table.n))
        got, after = guide.reference_mask(bits, guide.record(dfa, s, wide=True), wd, wa, table, fed, eos)
        # the rule, from the dense host table alone
        nxt = guide.DONE if fed == eos else dfa.walk(table.bytes_of(fed), s) if table.bytes_of(fed) else s
        assert after == nxt, (s, fed)
        cur = nxt if nxt >= 1 else guide.DONE
        for i in rng.integers(0, table.n, 50).tolist() + [eos]:
            if i == eos:
                ok = cur == guide.DONE or bool(dfa.accept[cur])
            else:
                ok = cur != guide.DONE and len(table.bytes_of(i)) > 0 and dfa.walk(table.bytes_of(i), cur) != 0
            assert got[i] == (bits[i] if ok else guide.NEG_INF), (s, fed, i)
        if narrow:
            want, after_n = guide.reference_mask(bits, guide.record(dfa, s), nd, na, table, fed, eos)
            assert np.array_equal(got, want) and after == after_n, s
    # a record out of range is DONE and not written: only EOS is left
    for rec in ([257, 0, 1, C], [257, S, S + 1, C], [257, S, 0, C], [257, S, 1, 0], [257, S, 1, 257], [257, 65535, 1, C], [257, 70000, 1, 1]):
        got, after = guide.reference_mask(bits, rec, wd, wa, table, 5, eos)
        assert after == rec[2] and got[eos] == bits[eos] and (np.delete(got, eos) == guide.NEG_INF).all(), rec
    got, after = guide.reference_mask(bits, [256, S, 1, C], wd, wa, table, 5, eos)                # the wide bit alone: inactive
    assert np.array_equal(got, bits) and after == 1


def test_check_and_replay_take_a_wide_guide():
    table, eos = _vocab_table()
    dfa = guide.compile_json(BOOK)
    assert guide.checked(dfa, table, eos) is dfa
    ids = [table.n - 7, 1 + ord("a"), 1 + ord("b"), table.n - 6, 1 + ord("7"), 1 + ord("}")]
    assert guide.replay_state(dfa, table, ids, eos) == dfa.walk(b'{"title":"ab","year":7}') and dfa.accept[dfa.walk(b'{"title":"ab","year":7}')]
    assert guide.replay_state(dfa, table, ids + [eos], eos) == guide.DONE
    only_digits = guide.VocabTable([b""] + [bytes([b]) for b in b"0123456789"])
    with pytest.raises(ValueError, match="cannot spell"):
        guide.check(dfa, only_digits, 0)


# ----------------------------------------------------------------------------- plumbing
def test_per_prompt_and_exclusion():
    s = {"type": "boolean"}
    assert guide.per_prompt(2, schema=s)[1].matches("true") and guide.per_prompt(2) is None
    got = guide.per_prompt(3, regex=["a", None, None], schema=[None, s, None])
    assert got[0].matches("a") and got[1].matches("false") and got[2] is None
    assert guide.per_prompt(1, schema='{"type": "null"}')[0].matches("null")
    assert guide.compile_guide(schema=s) is guide.compile_json(s) and guide.compile_guide() is None
    for kw in (dict(regex="a", schema=s), dict(choice=["a"], schema=s), dict(regex="a", choice=["a"], schema=s)):
        with pytest.raises(ValueError, match="exclude each other"):
            guide.compile_guide(**kw)
    with pytest.raises(ValueError, match="guided_regex and guided_choice exclude each other: give one per prompt"):
        guide.compile_guide(regex="a", choice=["a"])
    with pytest.raises(ValueError, match="exclude each other"):
        guide.per_prompt(2, regex=["a", None], schema=[s, None])
    with pytest.raises(ValueError, match="2 values for 3 prompts"):
        guide.per_prompt(3, schema=[s, None])
    with pytest.raises(ValueError, match="speculate"):
        guide.refuse_speculation(guide.per_prompt(1, schema=s), 2)


def test_request_record_and_engine_carrier():
    from phi_3_vision_mlx_amd.engine import guide_args
    from phi_3_vision_mlx_amd.request import GUIDE_ARGS, RequestOptions
    assert guide.FIELDS == ("regex", "choice", "schema")
    assert guide.request_guide({"schema": BOOK}) is guide.compile_json(BOOK) and guide.request_guide({"schema": json.dumps(BOOK)}) is guide.compile_json(BOOK)
    inputs = {"input_ids": np.arange(5)[None]}
    sent = guide_args(inputs, schema=BOOK)
    assert sent is not inputs and sent[GUIDE_ARGS] == {"schema": BOOK} and GUIDE_ARGS not in inputs
    opts = RequestOptions.read(sent)
    assert opts.guide == {"schema": BOOK}                                         # the dict travels unchanged
    checked = opts.checked([])
    assert checked.guide is guide.compile_json(BOOK) and checked.guide.n_states > 255

    class Eng:
        def submit(self, inputs, max_tokens, **kw):
            return inputs, kw
    got, kw = opts.send(Eng(), inputs, 4)
    assert got[GUIDE_ARGS] == {"schema": BOOK} and kw == {} and list(got[GUIDE_ARGS]["schema"]["properties"]) == ["title", "year"]
    for kw in (dict(regex="a", schema=BOOK), dict(choice=["b"], schema=BOOK)):
        with pytest.raises(ValueError, match="exclude each other"):
            guide_args(inputs, **kw)
    for bad in ({"json": "{}"}, {"json": BOOK}, {"schema": {"type": "string", "format": "date"}}, {"schema": 3}, {"schema": HUGE},
                {"schema": BOOK, "regex": "a"}):
        with pytest.raises(ValueError):
            RequestOptions(guide=bad).checked([])


def test_parse_guide_and_generate_kwargs():
    from phi_3_vision_mlx_amd.server import generate_kwargs, in_use, parse_guide
    assert parse_guide({"guided_json": BOOK}, 2) == [{"schema": BOOK}] * 2
    assert parse_guide({"guided_json": json.dumps(BOOK)}, 1) == [{"schema": json.dumps(BOOK)}]
    assert parse_guide({"guided_json": None, "response_format": None}, 1) is None
    fmt = {"type": "json_schema", "json_schema": {"name": "book", "schema": BOOK}}
    assert parse_guide({"response_format": fmt}, 1) == [{"schema": BOOK}]
    assert parse_guide({"response_format": {"type": "text"}}, 1) is None
    assert parse_guide({"response_format": {"type": "text"}, "guided_regex": "a"}, 1) == [{"regex": "a"}]
    for bad, word in (({"response_format": {"type": "json_object"}}, "free-form JSON is not a regular language"),
                      ({"response_format": {"type": "json_object"}}, "65536"),
                      ({"response_format": {"type": "json_schema"}}, "json_schema"), ({"response_format": {"type": "xml"}}, "xml"),
                      ({"response_format": "json"}, "response_format"), ({"response_format": fmt, "guided_json": BOOK}, "exclude each other"),
                      ({"response_format": fmt, "guided_regex": "a"}, "exclude each other"),
                      ({"guided_json": BOOK, "guided_regex": "a"}, "exclude each other"), ({"guided_json": BOOK, "guided_choice": ["a"]}, "exclude each other"),
                      ({"guided_json": 3}, "guided_json"), ({"guided_json": [BOOK]}, "guided_json"), ({"guided_json": "{"}, "not valid JSON"),
                      ({"guided_json": {"type": "integer", "minimum": 1}}, "minimum"), ({"guided_json": HUGE}, "at most 65536")):
        with pytest.raises(ValueError, match=word):
            parse_guide(bad, 1)
    assert in_use(guide=[{"schema": BOOK}]) == {"guide": [{"schema": BOOK}]}
    assert generate_kwargs(None, None, None, None, None, None, 0, 2, [{"schema": BOOK}, None]) == {"guided_json": [BOOK, None]}
    assert generate_kwargs(None, None, None, None, None, None, 0, 2, [{"schema": BOOK}, {"regex": "b"}]) == \
        {"guided_regex": [None, "b"], "guided_json": [BOOK, None]}
    assert generate_kwargs(None, None, None, None, 2, None, 0, 1, [{"schema": BOOK}]) == {"guided_json": BOOK, "n": 2, "best_of": None}
    assert generate_kwargs(None, None, None, None, None, None, 3, 1, [{"schema": BOOK}]) == {"speculate": 3}


def test_server_carries_the_schema_and_answers_400():
    import threading
    import urllib.error
    import urllib.request
    from phi_3_vision_mlx_amd.server import serve
    calls = []

    def fake_generate(prompts, max_tokens, images=None, **kw):
        calls.append(kw)
        return [f"{p}|{max_tokens}" for p in prompts]

    def post(body):
        req = urllib.request.Request(f"http://127.0.0.1:{port}/v1/completions", data=json.dumps(body).encode(),
                                     headers={"Content-Type": "application/json"})
        with urllib.request.urlopen(req, timeout=10) as r:
            return r.status, json.loads(r.read())
    httpd, engine = serve(fake_generate, port=0, host="127.0.0.1", merge=False, max_tokens_cap=1000, vocab_size=64, speculate=True,
                          speculate_default=4)
    threading.Thread(target=httpd.serve_forever, daemon=True).start()
    port = httpd.server_address[1]
    try:
        assert post({"prompt": ["a", "b"], "max_tokens": 5, "guided_json": BOOK})[0] == 200
        assert calls[-1] == {"guide": [{"schema": BOOK}] * 2} and list(calls[-1]["guide"][0]["schema"]["properties"]) == ["title", "year"]
        assert post({"prompt": "c", "max_tokens": 5, "response_format": {"type": "json_schema", "json_schema": {"schema": BOOK}}})[0] == 200
        assert calls[-1] == {"guide": [{"schema": BOOK}]}
        assert post({"prompt": "c", "max_tokens": 5, "response_format": {"type": "text"}, "temperature": 0})[0] == 200
        assert "guide" not in calls[-1]
        for bad, word in (({"guided_json": {"type": "object"}}, "properties"), ({"guided_json": {"type": "string", "pattern": "a"}}, "pattern"),
                          ({"guided_json": HUGE}, "at most 65536"), ({"response_format": {"type": "json_object"}}, "not a regular language"),
                          ({"guided_json": BOOK, "speculate": 4}, "speculative"), ({"guided_json": "{{"}, "not valid JSON")):
            n = len(calls)
            with pytest.raises(urllib.error.HTTPError) as e:
                post(dict({"prompt": "x", "max_tokens": 3}, **bad))
            assert e.value.code == 400 and word in json.loads(e.value.read())["error"], bad
            assert len(calls) == n
    finally:
        httpd.shutdown()
        engine.close()
