"""What a JSON-schema guide costs on the host: guide.compile_json (schema -> pattern -> NFA -> minimised DFA over byte classes) and
guide.check against a 32,064-entry vocabulary table, cold and from the caches, for five schemas of 78 to 698 states.  One CPU thread;
both run in the thread that submits the request.  No GPU.  The vocabulary is synthetic (no real tokenizer is on disk): 3 specials,
the 256 single bytes, then random pieces of 1..8 bytes over letters, digits, space and JSON punctuation; id 32007 is the EOS.

    python tools/guide_json_compile_time.py [--reps 3]      (the output is profiles/guide_json_compile.txt)
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from phi_3_vision_mlx_amd import guide  # noqa: E402

N, EOS = 32064, 32007


def S(**k):
    return dict({"type": "string"}, **k)


def obj(**p):
    return {"type": "object", "properties": p, "required": list(p)}


I, B = {"type": "integer"}, {"type": "boolean"}
SCHEMAS = {
    "name / age / email": obj(name=S(), age=I, email=S()),
    "... + tags[<= 4] + active": obj(name=S(), age=I, email=S(), tags={"type": "array", "items": S(), "maxItems": 4}, active=B),
    "tool call: 4 tools, 3 arguments": obj(tool={"enum": ["search", "lookup", "add_event", "send_mail"]}, arguments=obj(query=S(), limit=I, exact=B)),
    "title (maxLength 32) / year": obj(title=S(maxLength=32), year=I),
    "nested object + array[<= 4] of 3-field objects": obj(owner=obj(name=S(maxLength=26), id=I), entries={
        "type": "array", "maxItems": 4, "items": obj(label=S(), count=I, kept=B)}),
}


def table():
    rng = np.random.default_rng(0)
    alpha = np.frombuffer(b'abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789 {}[]":,.-_\\/', dtype=np.uint8)
    strings = [b""] * 3 + [bytes([b]) for b in range(256)]
    while len(strings) < N:
        strings.append(bytes(rng.choice(alpha, int(rng.integers(1, 9))).tolist()))
    strings[EOS] = b""
    t = guide.VocabTable(strings)
    t.padded()
    return t


def clock(fn):
    t = time.perf_counter()
    out = fn()
    return time.perf_counter() - t, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3, help="cold repetitions per schema (the caches are emptied before each); medians")
    a = ap.parse_args()
    tab = table()
    print(f"vocabulary table: {tab.n} ids, {tab.n_bytes} bytes; medians of {a.reps} cold repetitions, min .. max in brackets")
    print(f"{'schema':48s} {'states':>6s} {'classes':>7s} {'form':>6s} {'compile, cold (ms)':>26s} {'cached (us)':>12s} {'check, cold (ms)':>26s} {'cached (us)':>12s}")
    for name, schema in SCHEMAS.items():
        cold, hit, chk, chk_hit = [], [], [], []
        for _ in range(a.reps):
            guide._cache.clear()
            guide._checked.clear()
            t, dfa = clock(lambda: guide.compile_json(schema))
            cold.append(t * 1e3)
            hit.append(clock(lambda: guide.compile_json(schema))[0] * 1e6)
            chk.append(clock(lambda: guide.checked(dfa, tab, EOS))[0] * 1e3)
            chk_hit.append(clock(lambda: guide.checked(dfa, tab, EOS))[0] * 1e6)
        span = lambda v: f"{statistics.median(v):8.1f} [{min(v):7.1f} .. {max(v):7.1f}]"      # noqa: E731
        print(f"{name:48s} {dfa.n_states:6d} {dfa.n_classes:7d} {'wide' if guide.is_wide(dfa) else 'narrow':>6s} {span(cold)} "
              f"{statistics.median(hit):12.1f} {span(chk)} {statistics.median(chk_hit):12.1f}")


if __name__ == "__main__":
    main()
