"""Records what the decoder's projection layer does on the host, for every weight format -- the fixture of
tests/test_proj_calls_cpu.py (tests/golden/proj_calls.json).  No GPU, no library: the ops are replaced by loggers.

    python tests/golden/gen_golden_proj_calls.py          # rewrites tests/golden/proj_calls.json
    python tests/golden/gen_golden_proj_calls.py --time   # host cost of one Phi3VModel._proj_frozen call on the shell below

Two recordings, both through interfaces that did not change when the weight handle was stated once (ops._weight_format, Phi3VModel._handle):
  "chooser"  Phi3VModel._proj_frozen on a model shell with `meta` tensors: which ops it calls, in order, and which of them were given
             `norm_w`, over STATES x ROWS x KS x MS x EPILOGUES x {norm_w absent, present}; the 4-bit state again under
             P3V_Q4_ROWS=0 and under P3V_Q4_ROWS8_NORM=0; and a packed copy whose bf16 matrix was replaced.  One symbol per case
             against the table of distinct sequences, in the nesting order of `grid()`.
  "launch"   ops.gemv / gemv_fp8 / gemv_q4 / gemv_b13 / gemv_step_begin / gemv_step_end on small CPU tensors with a stand-in
             library: the entry symbol, the argument struct's type and every field (a pointer as the role of the tensor it came
             from), the `_chk` calls, the name given to `L.check`, and the shape and dtype of an `out` the wrapper allocated.
"""
import contextlib
import ctypes as C
import itertools
import json
import os
import statistics
import sys
import time
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PATH = os.path.join(ROOT, "tests", "golden", "proj_calls.json")
KEY = "model.layers.0.mlp.gate_up_proj.weight"
BF16, F32, I32, U8 = torch.bfloat16, torch.float32, torch.int32, torch.uint8

STATES = ("bf16", "b13", "b13_silu", "fp8", "fp8_act", "q4")
ROWS = (16, 24, 64, 96, 256, 512)
KS = (3072, 8192, 1024, 576, 520)
MS = (1, 2, 8, 9, 16, 17, 64)
EPILOGUES = ("EPI_NONE", "EPI_RESID_BF16", "EPI_SILU_MUL")
KNOBS = ("P3V_Q4_ROWS", "P3V_Q4_ROWS8_NORM")
SYMBOLS = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ"


def grid():
    return itertools.product(ROWS, KS, MS, EPILOGUES, (False, True))


@contextlib.contextmanager
def patched(obj, **attrs):
    old = {k: getattr(obj, k) for k in attrs}
    for k, v in attrs.items():
        setattr(obj, k, v)
    try:
        yield
    finally:
        for k, v in old.items():
            setattr(obj, k, v)


@contextlib.contextmanager
def environ(name, value):
    old = os.environ.get(name)
    os.environ[name] = value
    try:
        yield
    finally:
        if old is None:
            del os.environ[name]
        else:
            os.environ[name] = old


# ------------------------------------------------------------------ recording "chooser"
def shell(state, rows, K, device="meta"):
    """A Phi3VModel that was never constructed, holding one matrix of `rows` x K in the given weight state."""
    from phi_3_vision_mlx_amd import ops
    from phi_3_vision_mlx_amd.model import Phi3VModel
    m = Phi3VModel.__new__(Phi3VModel)
    m.cfg = types.SimpleNamespace(rms_norm_eps=1e-5)
    m.w, m.w8, m.w4, m.w13, m.adapters, m._bank, m.epoch = {}, {}, {}, {}, {}, {}, 0
    m.fp8_act = state == "fp8_act"
    m._deq = torch.empty(rows * K, dtype=BF16, device=device)
    if state in ("bf16", "b13", "b13_silu", "b13_stale"):
        m.w[KEY] = torch.empty((rows, K), dtype=BF16, device=device)
    if state in ("b13", "b13_silu", "b13_stale"):
        src = torch.empty((rows, K), dtype=BF16, device=device) if state == "b13_stale" else m.w[KEY]
        m.w13[KEY] = ops.PackedB13(torch.empty((rows, K * 13 // 8), dtype=U8, device=device), 100, rows, K, state == "b13_silu", src=src)
        m._keep = src                                             # (the packed copy holds its source weakly)
    if state in ("fp8", "fp8_act"):
        m.w8[KEY] = (torch.empty((rows, K), dtype=U8, device=device), torch.empty((rows,), dtype=F32, device=device))
    if state == "q4":
        m.w4[KEY] = (torch.empty((rows, K // 8), dtype=I32, device=device), torch.empty((rows, K // 64), dtype=I32, device=device))
    return m


def op_loggers(log):
    """Stand-ins for the ops _proj_frozen may call: each appends its name, and a `+` when it was given a norm weight."""
    def note(name, normed):
        log.append(name + ("+" if normed else ""))

    def gemv_like(name):
        def f(*a, norm_w=None, **kw):
            note(name, norm_w is not None)
            return name
        return f

    def quant_fp8_rows(x, norm_w=None, norm_eps=0.0, out=None, scale=None):
        note("quant_fp8_rows", norm_w is not None)
        return "a8", "a_scale"

    def rmsnorm(x, w, eps, out=None):
        note("rmsnorm", w is not None)
        return x

    fns = {name: gemv_like(name) for name in ("gemv", "gemv_fp8", "gemv_q4", "gemv_b13", "gemm", "gemm_fp8", "dequant_q4", "dequant_fp8")}
    fns.update(quant_fp8_rows=quant_fp8_rows, rmsnorm=rmsnorm)
    return fns


def chooser_case(ops, m, log, M, K, epilogue, normed):
    del log[:]
    x = torch.empty((M, K), dtype=BF16, device="meta")
    norm_w = torch.empty((K,), dtype=BF16, device="meta") if normed else None
    m._proj_frozen(x, KEY, getattr(ops, epilogue), None, norm_w, None, torch.empty((M, K), dtype=BF16, device="meta"))
    return ",".join(log)


def record_chooser():
    from phi_3_vision_mlx_amd import ops
    log, table, cases = [], [], {}

    def run(state):
        symbols = []
        for (rows, K), sub in itertools.groupby(grid(), key=lambda c: c[:2]):
            m = shell(state, rows, K)
            for _, _, M, epilogue, normed in sub:
                seq = chooser_case(ops, m, log, M, K, epilogue, normed)
                if seq not in table:
                    table.append(seq)
                symbols.append(SYMBOLS[table.index(seq)])
        return "".join(symbols)

    with patched(ops, **op_loggers(log)):
        for state in STATES:
            cases[state] = run(state)
        for knob in KNOBS:
            with environ(knob, "0"):
                cases[f"q4,{knob}=0"] = run("q4")
        m = shell("b13_stale", 64, 3072)                         # the bf16 matrix is not the one the copy was packed from
        stale = {"sequence": chooser_case(ops, m, log, 1, 3072, "EPI_NONE", True), "in_w13": KEY in m.w13, "epoch": m.epoch}
    return {"axes": {"state": list(cases), "rows": ROWS, "K": KS, "M": MS, "epilogue": EPILOGUES, "norm_w": [False, True]},
            "sequences": dict(zip(SYMBOLS, table)), "cases": cases, "stale_copy": stale}


def time_chooser(repeats=15, calls=20000):
    """Median (and min .. max) over `repeats` timings of one _proj_frozen call, per weight state, in microseconds."""
    from phi_3_vision_mlx_amd import ops
    out = {}
    with patched(ops, **op_loggers([])):
        for state, M in (("bf16", 1), ("b13", 1), ("fp8", 1), ("q4", 1), ("bf16", 16), ("q4", 8), ("fp8_act", 64), ("fp8", 64), ("q4", 64)):
            m = shell(state, 256, 3072)
            x, norm_w = torch.empty((M, 3072), dtype=BF16, device="meta"), torch.empty((3072,), dtype=BF16, device="meta")
            times = []
            for _ in range(repeats):
                t0 = time.perf_counter()
                for _ in range(calls):
                    m._proj_frozen(x, KEY, ops.EPI_NONE, None, norm_w, None, x)
                times.append((time.perf_counter() - t0) / calls * 1e6)
            out[f"{state},M={M}"] = (statistics.median(times), min(times), max(times))
    return out


# ------------------------------------------------------------------ recording "launch"
class Library:
    """Stands in for libp3v.so: every entry notes its symbol and arguments and answers `rc`."""

    def __init__(self, rc=0):
        self.calls, self.rc = [], rc

    def __getattr__(self, symbol):
        def entry(*args):
            self.calls.append((symbol, args))
            return self.rc
        return entry


def handles(silu_pairs=False, rows=8, K=64):
    """format -> (the weight handle, its tensors by role)."""
    from phi_3_vision_mlx_amd import ops
    w = torch.zeros((rows, K), dtype=BF16)
    w8, ws = torch.zeros((rows, K), dtype=U8), torch.zeros((rows,), dtype=F32)
    w4, sb = torch.zeros((rows, K // 8), dtype=I32), torch.zeros((rows, K // 64), dtype=I32)
    data = torch.zeros((rows, K * 13 // 8), dtype=U8)
    return {"bf16": (w, {"w": w}), "fp8": ((w8, ws), {"w8": w8, "w_scale": ws}), "q4": ((w4, sb), {"w4": w4, "sb": sb}),
            "b13": (ops.PackedB13(data, 3, rows, K, silu_pairs), {"data": data})}


def struct_fields(ref, roles):
    s = ref._obj
    vals = []
    for name, ctype in s._fields_:
        v = getattr(s, name)
        vals.append((roles[v] if v else None) if ctype is C.c_void_p else v)
    return [type(s).__name__] + vals


def launch_case(ops, call, tensors, rc=0):
    """Run `call` against the stand-in library; the record of what reached it."""
    lib, chk, checked = Library(rc), [], []
    roles = {t.data_ptr(): role for role, t in tensors.items() if t is not None}
    assert len(roles) == sum(t is not None for t in tensors.values())

    def _chk(t, dtype, name):
        chk.append(f"{name}:{str(dtype)[6:]}")
        return t

    with patched(ops, _chk=_chk, _stream=lambda: 0), patched(ops.L, lib=lambda: lib, check=lambda code, what="": checked.append(what)):
        try:
            ret = call()
        except ValueError as e:
            return {"raises": str(e), "chk": chk, "launched": len(lib.calls)}
    rec = {"chk": chk, "check": checked}
    if torch.is_tensor(ret):
        given = ret.data_ptr() in roles
        rec["returns"] = roles[ret.data_ptr()] if given else [list(ret.shape), str(ret.dtype)[6:]]
        roles.setdefault(ret.data_ptr(), "allocated")
    else:
        rec["returns"] = ret
    rec["calls"] = [[symbol] + [struct_fields(a, roles) if hasattr(a, "_obj") else a for a in args] for symbol, args in lib.calls]
    return rec


def record_launch():
    from phi_3_vision_mlx_amd import ops
    plain = {"bf16": ops.gemv, "fp8": ops.gemv_fp8, "q4": ops.gemv_q4, "b13": ops.gemv_b13}
    M, K, rows, V, half, tab_t, steps = 2, 64, 8, 12, 4, 6, 5
    cases = {}

    def parts(fmt, handle):
        return (handle,) if fmt in ("bf16", "b13") else handle

    for fmt, epilogue, normed, with_resid, with_out in itertools.product(plain, EPILOGUES + ("EPI_F32",), (0, 1), (0, 1), (0, 1)):
        handle, t = handles(silu_pairs=epilogue == "EPI_SILU_MUL")[fmt]
        n = rows // 2 if epilogue == "EPI_SILU_MUL" else rows
        t.update(x=torch.zeros((M, K), dtype=BF16), norm_w=torch.zeros((K,), dtype=BF16) if normed else None,
                 resid=torch.zeros((M, n), dtype=BF16) if with_resid else None,
                 out=torch.zeros((M, n), dtype=F32 if epilogue == "EPI_F32" else BF16) if with_out else None)
        cases[f"{fmt},{epilogue},norm_w={normed},resid={with_resid},out={with_out}"] = launch_case(
            ops, lambda: plain[fmt](t["x"], *parts(fmt, handle), getattr(ops, epilogue), resid=t["resid"], norm_w=t["norm_w"], norm_eps=0.25,
                                    out=t["out"]), t)

    def begin(handle, t, table_k=K):
        t.update(tok=torch.zeros((1,), dtype=I32), table=torch.zeros((V, table_k), dtype=BF16), x_out=torch.zeros((1, table_k), dtype=BF16),
                 cos_t=torch.zeros((1, tab_t, half)), sin_t=torch.zeros((1, tab_t, half)), d_past=torch.zeros((1,), dtype=I32),
                 cos_out=torch.zeros((1, half)), sin_out=torch.zeros((1, half)))
        return lambda: ops.gemv_step_begin(t["tok"], t["table"], t["x_out"], t["cos_t"], t["sin_t"], t["d_past"], t["cos_out"], t["sin_out"],
                                           handle, t["norm_w"], 0.25, t["out"])

    def end(handle, t, x_k=K, ws_bytes=None):
        t.update(x=torch.zeros((1, x_k), dtype=BF16), next_tok=torch.zeros((1,), dtype=I32), tok=torch.zeros((1,), dtype=I32),
                 history=torch.zeros((1, steps), dtype=I32), d_step=torch.zeros((1,), dtype=I32), d_past=torch.zeros((1,), dtype=I32),
                 ticket=torch.zeros((1,), dtype=I32),
                 amax_ws=torch.zeros((ops.L.GEMV_STEP_WS_BYTES if ws_bytes is None else ws_bytes,), dtype=U8))
        return lambda: ops.gemv_step_end(t["x"], handle, t["norm_w"], 0.25, t["out"], t["next_tok"], t["tok"], t["history"], t["d_step"],
                                         t["d_past"], t["ticket"], t["amax_ws"])

    for which, fmt, normed, with_out in itertools.product((begin, end), plain, (0, 1), (0, 1)):
        handle, t = handles()[fmt]
        t.update(norm_w=torch.zeros((K,), dtype=BF16) if normed else None, out=torch.zeros((1, rows), dtype=BF16) if with_out else None)
        cases[f"{fmt},step_{which.__name__},norm_w={normed},out={with_out}"] = launch_case(ops, which(handle, t), t)

    for fmt in plain:                                            # the library keeps the separate launch: the wrappers answer False
        for which in (begin, end):
            handle, t = handles()[fmt]
            t.update(norm_w=torch.zeros((K,), dtype=BF16), out=torch.zeros((1, rows), dtype=BF16))
            cases[f"{fmt},step_{which.__name__},unsupported"] = launch_case(ops, which(handle, t), t, rc=ops.L.ERR_UNSUPPORTED)
        handle, t = handles()[fmt]                                # the step's last projection checks its arg-max workspace
        t.update(norm_w=torch.zeros((K,), dtype=BF16), out=torch.zeros((1, rows), dtype=BF16))
        cases[f"{fmt},step_end,small_amax_ws"] = launch_case(ops, end(handle, t, ws_bytes=64), t)

    handle, t = handles()["b13"]                                  # the packed format knows its K: a mismatch is refused
    t.update(x=torch.zeros((M, K + 8), dtype=BF16), norm_w=None, out=None)
    cases["b13,EPI_NONE,K_mismatch"] = launch_case(ops, lambda: ops.gemv_b13(t["x"], handle), t)
    t.update(norm_w=torch.zeros((K,), dtype=BF16), out=torch.zeros((1, rows), dtype=BF16))
    cases["b13,step_begin,K_mismatch"] = launch_case(ops, begin(handle, t, table_k=K + 8), t)
    cases["b13,step_end,K_mismatch"] = launch_case(ops, end(handle, t, x_k=K + 8), t)
    return cases


def record_all():
    return {"chooser": record_chooser(), "launch": record_launch()}


def dumps(rec):
    """One case per line: compact, and a change shows up as the lines of the cases it touches."""
    lines = []
    for part, groups in rec.items():
        for group, value in groups.items():
            if part == "chooser" and group in ("sequences", "cases"):
                lines += [json.dumps([part, group, k, v], separators=(",", ":")) for k, v in value.items()]
            else:
                lines.append(json.dumps([part, group, value], separators=(",", ":")))
    return "[\n" + ",\n".join(lines) + "\n]\n"


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    if "--time" in sys.argv:
        for case, (med, lo, hi) in time_chooser().items():
            print(f"{case:14s} median {med:6.3f} us  (min {lo:6.3f}, max {hi:6.3f})")
        sys.exit(0)
    text = dumps(record_all())
    with open(PATH, "w") as f:
        f.write(text)
    print(f"wrote {PATH}: {len(text)} bytes")
