"""Repetition / presence / frequency penalties and logit_bias on the MI355X: p3v_penalize and p3v_penalty_note against the NumPy
restatement of the rule (penalties.reference_adjust, penalties.seen_table) BIT FOR BIT -- every operation of the rule is one
correctly rounded fp32 operation, so there is no tolerance; NaNs compare as "is NaN" --, then the penalised captures of the model
through api.generate (each emitted token is the first maximum of the restatement applied to that step's own raw logits, with the
table rebuilt on the host: one run, teacher-forced against itself), graph against eager launches, sampled rows across batch
sizes, log-probabilities of the raw logits, and the continuous engine with refilled slots."""
import math

import numpy as np
import pytest
import torch

from phi_3_vision_mlx_amd import penalties

pytestmark = pytest.mark.gpu
INF = float("inf")
N = 32064
EOS = 32007
CANARY16 = 0x7FD5                                   # a NaN payload no computation produces: "never written"


def _bf16_dev(bits):
    return torch.as_tensor(np.ascontiguousarray(bits).view(np.int16)).view(torch.bfloat16).cuda()


def _bits_of(t):
    return t.detach().contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _i32(v):
    """int32 on the device; uint32 words travel as their bits"""
    a = np.ascontiguousarray(v)
    return torch.as_tensor(a.view(np.int32) if a.dtype == np.uint32 else a.astype(np.int32)).cuda()


def _u32_of(t):
    return t.detach().contiguous().cpu().numpy().view(np.uint32)


def assert_rows_equal(got, want, what):
    """bit equality, NaNs as "is NaN" """
    got, want = np.asarray(got, dtype=np.uint16), np.asarray(want, dtype=np.uint16)
    gn, wn = (got & 0x7FFF) > 0x7F80, (want & 0x7FFF) > 0x7F80
    assert np.array_equal(gn, wn), (what, "NaN positions", np.nonzero(gn != wn)[0][:8])
    bad = np.nonzero((got != want) & ~gn)[0]
    assert bad.size == 0, (what, bad[:8], got[bad[:8]], want[bad[:8]])


# rows of one launch: inactive, repetition only, all three, bias only (+ variations when there are more rows)
RECORDS = [(1.3, 0.5, 0.5, 0), (1.3, 0.0, 0.0, 1), (1.3, 0.5, 0.25, 3), (1.0, 0.0, 0.0, 3), (0.75, -0.125, 2.0, 1),
           (1.0, 0.1, 0.0, 1), (2.5, 0.0, 1e30, 1), (1.3, 0.5, 0.5, 2)]


def _case(n, rows, seed):
    """logits bits, seen words, bias and records built to fail: specials in every row, a NaN payload in the inactive row"""
    rng = np.random.default_rng(seed)
    bits = penalties.f32_to_bf16_bits(rng.normal(0, 4.0, (rows, n)).astype(np.float32))
    seen = np.zeros((rows, n), dtype=np.uint32)
    kinds = rng.integers(0, 6, (rows, n))
    seen[kinds == 1] = 0x80000000                                             # prompt only
    seen[kinds == 2] = rng.integers(1, 9, int((kinds == 2).sum())).astype(np.uint32)                  # output only
    seen[kinds == 3] = np.uint32(0x80000000) | rng.integers(1, 400, int((kinds == 3).sum())).astype(np.uint32)   # both
    bias = rng.normal(0, 2.0, (rows, n)).astype(np.float32)
    bias[rng.random((rows, n)) < 0.02] = -INF
    bias[rng.random((rows, n)) < 0.5] = 0.0
    special = [0x0000, 0x8000, 0x7F80, 0xFF80, 0x7F7F, 0xFF7F, 0x0080, 0x3F80]   # +-0, +-inf, +-largest finite, smallest normal, 1
    for r in range(rows):
        for k, s in enumerate(special):
            for j, word in enumerate((0, 0x80000000, 3, 0x7FFFFFFF)):          # every special under every kind of seen word
                i = (k * 4 + j) * 7 % n
                if n > len(special) * 4 * 7:
                    bits[r, i], seen[r, i] = s, word
        bits[r, n - 1] = 0x7FC0 if r % 2 else bits[r, n - 1]                      # a NaN in the tail of odd rows
        seen[r, n // 2] = 0x7FFFFFFF
    off = 2 if rows == 1 else 0                                                   # (one row: the one with everything)
    recs = [RECORDS[(r + off) % len(RECORDS)] for r in range(rows)]
    if rows > 1:
        bits[0, min(5, n - 1)] = 0x7FA5                                           # inactive row: a NaN with a payload, kept
        bits[0, 0] = 0x8000
    return bits, seen, bias, recs


def _pack(recs):
    rows = [(rp, fp, pp, None) for rp, fp, pp, _ in recs]
    t = penalties.pack(rows)
    for i, r in enumerate(recs):
        t[i, 3] = r[3]
    return t.cuda()


def _ref(bits, recs, seen, bias):
    return np.stack([penalties.reference_adjust(bits[r], recs[r], seen[r], None if bias is None else bias[r]) for r in range(len(recs))])


# ---------------------------------------------------------------------------------------------------- p3v_penalize
@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("pad", [0, 3], ids=["aligned", "stride+3"])
@pytest.mark.parametrize("rows", [1, 3, 16])
@pytest.mark.parametrize("n", [1, 1037, N])
def test_penalize_equals_the_restatement_bit_for_bit(n, rows, pad, with_bias):
    from phi_3_vision_mlx_amd import ops
    bits, seen, bias, recs = _case(n, rows, 1000 * rows + n + pad)
    stride, o_stride = n + pad, n + pad + 8                                       # out_stride != row_stride, same alignment class
    wide = np.full((rows, stride), 0x7FC0, dtype=np.uint16)
    wide[:, :n] = bits
    swide = np.zeros((rows, stride), dtype=np.uint32)
    swide[:, :n] = seen
    bwide = np.full((rows, stride), np.nan, dtype=np.float32)
    bwide[:, :n] = bias
    d_logits, d_seen = _bf16_dev(wide), _i32(swide)
    d_bias = torch.as_tensor(bwide).cuda() if with_bias else None
    out = _bf16_dev(np.full((rows, o_stride), CANARY16, dtype=np.uint16))
    got = ops.penalize(d_logits[:, :n], _pack(recs), d_seen[:, :n], None if d_bias is None else d_bias[:, :n], None, out=out[:, :n])
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    full = _bits_of(out).reshape(rows, o_stride)
    assert (full[:, n:] == CANARY16).all()                                        # nothing written beyond a row's n
    assert np.array_equal(_bits_of(d_logits).reshape(rows, stride), wide)         # the raw logits stay raw
    assert np.array_equal(_u32_of(d_seen).reshape(rows, stride), swide)           # fed = NULL: the table is only read
    want = _ref(bits, recs, seen, bias if with_bias else None)
    for r in range(rows):
        assert_rows_equal(full[r, :n], want[r], (n, rows, pad, with_bias, r))
    for r in range(rows):
        if not recs[r][3] & 1:
            assert np.array_equal(full[r, :n], bits[r])                           # an inactive row: bytes, payload and -0 included
    if n > 1 and rows > 2:
        assert not np.array_equal(full[2, :n], bits[2])                           # (and the active ones did change)


def test_penalize_counts_the_fed_token_before_it_adjusts():
    from phi_3_vision_mlx_amd import ops
    n = 1037
    tail0 = n - n % 8                                                             # first index of the element-by-element tail
    feds = [-1, n, 0, n - 1, tail0, 77, 77, 77, 2 ** 31 - 1, -(2 ** 31)]
    rows = len(feds)
    rng = np.random.default_rng(3)
    bits = penalties.f32_to_bf16_bits(rng.normal(2.0, 3.0, (rows, n)).astype(np.float32))
    seen = np.zeros((rows, n), dtype=np.uint32)
    seen[:, ::5] = 2
    seen[6, 77] = 0x80000000                                                      # prompt-only before: the bit stays, the count rises
    seen[7, 77] = 0x7FFFFFFF                                                      # a full count stays full
    recs = [(1.3, 0.5, 0.25, 1)] * rows
    recs[5] = (1.3, 0.5, 0.25, 0)                                                 # an inactive row counts nothing
    d_seen = _i32(seen)
    out = ops.penalize(_bf16_dev(bits), _pack(recs), d_seen, None, _i32(feds))
    torch.cuda.synchronize()
    after = _u32_of(d_seen).reshape(rows, n)
    want_seen = seen.copy()
    for r, f in enumerate(feds):
        if 0 <= f < n and recs[r][3] & 1 and (seen[r, f] & 0x7FFFFFFF) != 0x7FFFFFFF:
            want_seen[r, f] += 1
    assert np.array_equal(after, want_seen)                                       # exactly one count, only for in-range ids of active rows;
    assert after[6, 77] == 0x80000001 and after[2, 0] == 3 and after[3, n - 1] == 1 and after[4, tail0] == seen[4, tail0] + 1
    want = _ref(bits, recs, want_seen, None)                                      # ... two rows fed the same id do not touch each other,
    got = _bits_of(out).reshape(rows, n)                                          # and the adjusted value already sees the new count
    for r in range(rows):
        assert_rows_equal(got[r], want[r], r)
    before = _ref(bits, recs, seen, None)
    assert got[3, n - 1] != before[3, n - 1] and got[4, tail0] != before[4, tail0]


def test_penalize_refuses_bad_arguments():
    from phi_3_vision_mlx_amd import _lib, ops
    lib = _lib.lib()
    n = 64
    x = torch.zeros((2, n), dtype=torch.bfloat16, device="cuda")
    out = _bf16_dev(np.full((2, n), CANARY16, dtype=np.uint16))
    seen = torch.zeros((2, n), dtype=torch.int32, device="cuda")
    bias = torch.zeros((2, n), dtype=torch.float32, device="cuda")
    rec = _pack([RECORDS[1]] * 2)
    ids, first, count = _i32([[1, 2], [3, 4]]), _i32([0, 0]), _i32([2, 2])
    p = lambda a: a.data_ptr()                                                    # noqa: E731
    ok = (p(x), n, p(rec), p(seen), n, p(bias), n, None, p(out), n, 2, n, None)
    for i, bad in ((0, None), (2, None), (3, None), (8, None), (8, p(x)), (1, n - 1), (4, n - 1), (6, n - 1), (9, n - 1), (10, 0),
                   (10, 65536), (11, 0)):
        args = list(ok)
        args[i] = bad
        assert lib.p3v_penalize(*args) == -22, (i, bad)
    okn = (p(seen), n, p(ids), 2, p(first), p(count), 2, n, 1, 1, None)
    for i, bad in ((0, None), (2, None), (4, None), (5, None), (1, n - 1), (3, -1), (6, 0), (7, 0)):
        args = list(okn)
        args[i] = bad
        assert lib.p3v_penalty_note(*args) == -22, (i, bad)
    torch.cuda.synchronize()
    assert (_bits_of(out) == CANARY16).all() and int(seen.abs().sum()) == 0        # nothing was launched
    with pytest.raises((TypeError, ValueError)):
        ops.penalize(x, rec, seen.to(torch.int64))
    with pytest.raises(ValueError):
        ops.penalize(x, rec[:1], seen)
    with pytest.raises(ValueError):
        ops.penalize(x, rec, seen, bias[:, :32])


# ---------------------------------------------------------------------------------------------------- p3v_penalty_note
def test_penalty_note_scatter():
    from phi_3_vision_mlx_amd import ops
    n, rows, m = 1037, 5, 700
    rng = np.random.default_rng(9)
    ids = rng.integers(-5, n + 5, (rows, m)).astype(np.int32)                     # out-of-range and negative ids among them
    ids[0, :300] = 17                                                             # duplicates: a multiplicity of 300
    ids[1] = np.where(rng.random(m) < 0.5, n - 1, 0)
    first = np.array([0, 0, 650, 5, 123], dtype=np.int32)                         # a left-padded row, a run cut by the row's end
    count = np.array([m, m, 200, 0, 400], dtype=np.int32)                         # ... (row 2), count 0 (row 3)
    stale = np.full((rows + 1, n), 0xDEADBEEF, dtype=np.uint32)

    def host(as_prompt, base):
        out = base.copy()
        for r in range(rows):
            run = ids[r, first[r]:first[r] + count[r]]
            run = run[(run >= 0) & (run < n)]
            if as_prompt:
                out[r, run] |= np.uint32(0x80000000)
            else:
                np.add.at(out[r], run, np.uint32(1))
        return out

    # clear + prompt bits: the given rows are zeroed first (row `rows` is not given: untouched), a bit is set once
    seen = _i32(stale)
    ops.penalty_note(seen[:rows], _i32(ids), _i32(first), _i32(count), as_prompt=True, clear=True)
    torch.cuda.synchronize()
    got = _u32_of(seen).reshape(rows + 1, n)
    want = host(True, np.zeros((rows, n), dtype=np.uint32))
    assert np.array_equal(got[:rows], want) and (got[rows] == 0xDEADBEEF).all()
    assert got[0, 17] == 0x80000000 and not got[3].any()
    assert np.array_equal(got[0], penalties.seen_table(ids[0], [], n))
    # counts on top, no clear: multiplicities, the bits kept
    ops.penalty_note(seen[:rows], _i32(ids), _i32(first), _i32(count), as_prompt=False)
    torch.cuda.synchronize()
    got2 = _u32_of(seen).reshape(rows + 1, n)
    assert np.array_equal(got2[:rows], host(False, want)) and (got2[rows] == 0xDEADBEEF).all()
    mult = int((ids[0] == 17).sum())
    assert mult >= 300 and got2[0, 17] == 0x80000000 + mult                      # the count equals the multiplicity
    assert np.array_equal(got2[0], penalties.seen_table(ids[0], ids[0], n))
    # clear alone zeroes exactly the given rows (count 0 everywhere), a strided table included
    wide = _i32(np.full((3, n + 3), 0xDEADBEEF, dtype=np.uint32))
    ops.penalty_note(wide[1:, :n], _i32(ids[:2]), _i32([0, 0]), _i32([0, 0]), as_prompt=True, clear=True)
    torch.cuda.synchronize()
    w = _u32_of(wide).reshape(3, n + 3)
    assert not w[1:, :n].any() and (w[0] == 0xDEADBEEF).all() and (w[1:, n:] == 0xDEADBEEF).all()
    # n = 1
    one = _i32(np.array([[7]], dtype=np.uint32))
    ops.penalty_note(one, _i32([[0, 0, 1, -1]]), _i32([0]), _i32([4]), as_prompt=False, clear=True)
    assert _u32_of(one).tolist() == [[2]]


# ---------------------------------------------------------------------------------------------------- the model
@pytest.fixture(scope="module")
def tiny():
    from phi_3_vision_mlx_amd.api import load_synthetic
    model, proc = load_synthetic(tiny=True, seed=0, std_scale=4.0, device="cuda:0")
    yield model, proc
    del model
    torch.cuda.empty_cache()


PROMPT = "<|user|>\nTell me a story<|end|>\n<|assistant|>\n"
BATCH = ["<|user|>\nHi<|end|>\n<|assistant|>\n", "<|user|>\nA longer question here, padded left<|end|>\n<|assistant|>\n",
         "<|user|>\nWhy?<|end|>\n<|assistant|>\n", "<|user|>\nOne two three four<|end|>\n<|assistant|>\n"]
KW = dict(verbose=False, stream=False, mute=True)


def _gen(model, proc, prompt, **kw):
    """api._generate -> (per-row token lists, the returned text): the tokens as the streamer got them"""
    from phi_3_vision_mlx_amd import api
    steps = []

    class Rec(api.Streamer):
        def __call__(self, token):
            steps.append(api._rows(token))
            return super().__call__(token)
    orig, api.Streamer = api.Streamer, Rec
    try:
        text = api._generate(model, proc, prompt, **KW, **kw)
    finally:
        api.Streamer = orig
    return [list(col) for col in zip(*steps)], text


class _Watch:
    """the model's penalised entry points, with every call's raw logits and tokens kept"""

    def __init__(self, model):
        self.model, self.prefill, self.fed, self.logits, self.out, self.names, self.states = model, [], [], [], [], [], []
        self.orig = {k: getattr(model, k) for k in ("penal_step", "penal_logprob_step", "penalized_logits", "greedy_step")}

    def __enter__(self):
        def step(name):
            def f(token, cache):
                self.fed.append(token.reshape(-1).cpu().tolist())
                lg, tok = self.orig[name](token, cache)
                torch.cuda.synchronize()
                B = lg.shape[0]
                self.logits.append(_bits_of(lg).reshape(B, -1).copy())
                self.out.append(tok.reshape(-1).cpu().tolist())
                self.names.append(name)
                return lg, tok
            return f

        def plain(token, cache):
            self.states.append(cache[0].state)
            return self.orig["greedy_step"](token, cache)

        def first(st, logits, row0=0):
            self.states.append(st)
            last = logits[:, -1, :] if logits.dim() == 3 else logits
            self.prefill.append(_bits_of(last).reshape(last.shape[0], -1).copy())
            return self.orig["penalized_logits"](st, logits, row0)
        self.model.penal_step, self.model.penal_logprob_step, self.model.penalized_logits = step("penal_step"), step("penal_logprob_step"), first
        self.model.greedy_step = plain
        return self

    def __exit__(self, *a):
        for k in self.orig:
            self.model.__dict__.pop(k, None)


def _prompt_rows(proc, prompt):
    inputs = proc(prompt, None)
    ids = np.asarray(inputs["input_ids"])
    ids = ids[None] if ids.ndim == 1 else ids
    pads = (np.asarray(inputs["mask"]).reshape(ids.shape) == 0).sum(1) if "mask" in inputs else [0] * len(ids)
    return [ids[b, int(pads[b]):] for b in range(len(ids))]


def _check_teacher_forced(w, tokens, prompt_rows, rows):
    """every emitted token = the first maximum of the restatement on that step's own raw logits, the table rebuilt on the host"""
    V = w.prefill[0].shape[1]
    tables = penalties.bias_table(rows, V)
    for b, (toks, prow, row) in enumerate(zip(tokens, prompt_rows, rows)):
        rec = (row[0], row[1], row[2], penalties.flags(row))
        bias = None if tables is None else tables[b]
        for k, t in enumerate(toks):
            raw = w.prefill[0][b] if k == 0 else w.logits[k - 1][b]
            adj = penalties.reference_adjust(raw, rec, penalties.seen_table(prow, toks[:k], V), bias)
            vals = penalties.bf16_bits_to_f32(adj)
            assert not np.isnan(vals).any()
            assert t == int(np.argmax(vals)), (b, k, t, int(np.argmax(vals)))
            if k:
                assert w.fed[k - 1][b] == toks[k - 1]


def test_generate_greedy_follows_the_restatement_step_by_step(tiny):
    model, proc = tiny
    with _Watch(model) as w:
        toks, _ = _gen(model, proc, PROMPT, max_tokens=24, repetition_penalty=1.3, frequency_penalty=0.5, presence_penalty=0.5,
                       logit_bias={EOS: -INF})
    assert len(toks[0]) == 24 and len(w.out) == 23 and set(w.names) == {"penal_step"}
    rows = penalties.rows(1, 1.3, 0.5, 0.5, {EOS: -INF})
    prow = _prompt_rows(proc, PROMPT)
    _check_teacher_forced(w, toks, prow, rows)
    # the device table at the end: the prompt's bits and one count per FED token (all but the newest)
    st = w.states[0]
    seen = _u32_of(st.penalty["seen"]).reshape(1, -1)
    assert np.array_equal(seen[0], penalties.seen_table(prow[0], toks[0][:-1], seen.shape[1]))
    assert "penal_graph" in st.graphs["greedy"] and st.penalty["bias"] is not None


def test_generate_batch_left_padded_rows_keep_their_own_tables(tiny):
    model, proc = tiny
    rp, fp, pp = [1.3, 1.0, 1.6, 1.0], [0.5, 0.0, 0.0, 0.0], [0.5, 0.0, 0.25, 0.0]
    lb = [{EOS: -INF}, None, {EOS: -INF}, {EOS: -INF, 11: 2.0}]                     # row 1 plain, row 3 bias only
    with _Watch(model) as w:
        toks, _ = _gen(model, proc, BATCH, max_tokens=10, repetition_penalty=rp, frequency_penalty=fp, presence_penalty=pp, logit_bias=lb)
    rows = penalties.rows(4, rp, pp, fp, lb)
    prow = _prompt_rows(proc, BATCH)
    assert len({len(p) for p in prow}) > 1                                        # (rows ARE padded)
    _check_teacher_forced(w, toks, prow, rows)
    plain, _ = _gen(model, proc, BATCH, max_tokens=10)
    assert toks[1] == plain[1]                                                    # the plain row of a penalised batch: untouched
    seen = _u32_of(w.states[0].penalty["seen"]).reshape(4, -1)
    for b in (0, 2, 3):
        if EOS not in toks[b]:
            assert np.array_equal(seen[b], penalties.seen_table(prow[b], toks[b][:-1], seen.shape[1])), b   # (no pad id was noted)


def test_generate_logit_bias_bans_and_forces(tiny):
    model, proc = tiny
    plain, _ = _gen(model, proc, PROMPT, max_tokens=12)
    t0 = plain[0][0]
    banned, _ = _gen(model, proc, PROMPT, max_tokens=12, logit_bias={t0: -INF})
    assert t0 not in banned[0] and banned[0][0] != t0
    banned_s, _ = _gen(model, proc, PROMPT, max_tokens=12, logit_bias={str(t0): -INF}, temperature=1.5, seed=5)
    assert t0 not in banned_s[0]                                                  # sampled too: a banned token has weight 0
    forced, _ = _gen(model, proc, PROMPT, max_tokens=12, logit_bias={4242: 1e4})
    assert forced[0] == [4242] * 12


def test_generate_huge_presence_penalty_never_repeats(tiny):
    model, proc = tiny
    toks, _ = _gen(model, proc, PROMPT, max_tokens=17, presence_penalty=1e30, logit_bias={EOS: -INF})
    assert len(toks[0]) == 17 and len(set(toks[0])) == 17                          # 16 steps after the prefill token


def test_generate_defaults_are_todays_path(tiny):
    model, proc = tiny
    prompt = "<|user|>\nHello there, how are you<|end|>\n<|assistant|>\n"
    ref, ref_text = _gen(model, proc, prompt, max_tokens=10)
    with _Watch(model) as w:
        got, text = _gen(model, proc, prompt, max_tokens=10, repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0,
                         logit_bias=None)
        got2, _ = _gen(model, proc, prompt, max_tokens=10, logit_bias={}, repetition_penalty=[1.0])
    assert got == ref and got2 == ref and text == ref_text
    assert w.prefill == [] and w.names == [] and len(w.states) >= 2               # only the plain replay ran
    for s in w.states:
        assert s.penalty is None and s.sample_rows is None
        assert not {"penal_graph", "penal_logprob_graph", "sample_graph"} & set(s.graphs.get("greedy", {}))


def test_generate_refuses_speculation(tiny):
    from phi_3_vision_mlx_amd import api
    model, proc = tiny
    with pytest.raises(ValueError, match="speculate"):
        api._generate(model, proc, PROMPT, max_tokens=8, speculate=4, presence_penalty=0.5, **KW)
    with pytest.raises(ValueError, match="vocabulary"):
        api._generate(model, proc, PROMPT, max_tokens=8, logit_bias={N: 1.0}, **KW)


def test_captured_step_equals_eager_launches(tiny):
    """the same penalised request through the captured step and through eager model calls + p3v_penalize + p3v_sample"""
    from phi_3_vision_mlx_amd import ops, sampling
    model, proc = tiny
    rows = penalties.rows(1, 1.3, 0.5, 0.5, {EOS: -INF, 7: 1.5})
    inputs = proc(PROMPT, None)
    ids = np.asarray(inputs["input_ids"]).reshape(1, -1)
    V = model.cfg.vocab_size
    for srow in ((0.0, 0, 1.0, 0), (0.9, 50, 0.95, 11)):
        # captured
        logits, cache = model(**inputs, max_tokens=12)
        st = cache[0].state
        model.set_penalties(st, penalties.pack(rows), ids, 0, bias=penalties.bias_table(rows, V))
        tok = ops.sample(model.penalized_logits(st, logits), sampling.pack([srow], 0).cuda())[:, None]
        model.set_sampling(st, sampling.pack([srow], 1))
        graph = [tok.reshape(-1).cpu().tolist()]
        for _ in range(8):
            _, tok = model.penal_step(tok, cache)
            graph.append(tok.reshape(-1).cpu().tolist())
        # eager: the same kernels, launched one by one on buffers of this test
        logits, cache = model(**inputs, max_tokens=12)
        rec, srec = penalties.pack(rows).cuda(), sampling.pack([srow], 0).cuda()
        seen = torch.zeros((1, V), dtype=torch.int32, device="cuda")
        ops.penalty_note(seen, _i32(ids), _i32([0]), _i32([ids.shape[1]]), as_prompt=True, clear=True)
        bias = torch.as_tensor(penalties.bias_table(rows, V)).cuda()
        tok = ops.sample(ops.penalize(logits[:, -1, :], rec, seen, bias), srec)[:, None]
        eager = [tok.reshape(-1).cpu().tolist()]
        for _ in range(8):
            logits, cache = model(input_ids=tok, cache=cache)
            tok = ops.sample(ops.penalize(logits[:, -1, :], rec, seen, bias, tok.reshape(-1).contiguous()), srec)[:, None]
            eager.append(tok.reshape(-1).cpu().tolist())
        assert graph == eager, srow


def test_sampled_penalised_row_is_independent_of_its_batch(tiny):
    """temperature 0.8, seed 7 with penalties: the same tokens at B = 1 as as row 2 of a B = 4 batch whose other rows are plain,
    sampled only and bias only.  The rule makes a token a function of the row's logits, record and table alone, so the
    comparison needs the row's LOGITS to be the same bits in both runs, which the model gives for a row that carries no left
    padding: row 2 is the batch's longest prompt (the other three are padded, so the sampled batch also skips pad ids).  A
    left-padded row's prefill logits differ from its solo run's before this feature exists (measured on the tiny model: 26,926
    of 32,064 logits, by up to 0.064), and the plain sampled tokens with them; the test checks its premise first."""
    model, proc = tiny
    prompts = [BATCH[0], BATCH[2], BATCH[1], BATCH[3]]
    prows = _prompt_rows(proc, prompts)
    assert len(prows[2]) == max(len(p) for p in prows) and len({len(p) for p in prows}) > 1
    solo_logits, _ = model(**proc(prompts[2], None), max_tokens=10)
    batch_logits, _ = model(**proc(prompts, None), max_tokens=10)
    assert np.array_equal(_bits_of(solo_logits[0, -1]), _bits_of(batch_logits[2, -1]))     # the premise: the same prefill logits
    pen = dict(repetition_penalty=1.3, frequency_penalty=0.5, presence_penalty=0.5)
    solo, _ = _gen(model, proc, prompts[2], max_tokens=10, temperature=0.8, seed=7, **pen)
    # row 0 plain, row 1 sampled only, row 2 the request above, row 3 bias only
    batch, _ = _gen(model, proc, prompts, max_tokens=10, temperature=[0.0, 1.1, 0.8, 0.0], seed=[1, 2, 7, 3],
                    repetition_penalty=[1.0, 1.0, 1.3, 1.0], frequency_penalty=[0.0, 0.0, 0.5, 0.0], presence_penalty=[0.0, 0.0, 0.5, 0.0],
                    logit_bias=[None, None, None, {11: 3.0}])
    print("solo", solo[0], "batch row 2", batch[2])
    n = len(solo[0])
    assert n == 10 and batch[2][:n] == solo[0]
    unpenalised, _ = _gen(model, proc, prompts[2], max_tokens=10, temperature=0.8, seed=7)
    assert unpenalised[0] != solo[0]                                              # (the penalties do change this request's draws)
    plain, _ = _gen(model, proc, prompts, max_tokens=10, temperature=[0.0, 1.1, 0.8, 0.0], seed=[1, 2, 7, 3])
    assert batch[0] == plain[0] and batch[1] == plain[1]                          # the rows that did not ask


def test_logprobs_stay_those_of_the_raw_logits(tiny):
    from test_logprobs_cpu import assert_record, logprobs_ref
    from phi_3_vision_mlx_amd import api
    model, proc = tiny
    info = {}
    with _Watch(model) as w:
        toks, _ = _gen(model, proc, PROMPT, max_tokens=10, repetition_penalty=1.3, frequency_penalty=0.5, presence_penalty=0.5,
                       logit_bias={EOS: -INF}, logprobs=2, logprob_info=info)
    assert set(w.names) == {"penal_logprob_step"} and info["token_ids"][0] == toks[0]
    ranks = []
    for k, t in enumerate(toks[0]):
        raw = w.prefill[0][0] if k == 0 else w.logits[k - 1][0]
        rec = dict(token=t, logprob=info["token_logprobs"][0][k], rank=info["ranks"][0][k], top=info["top_logprobs"][0][k])
        assert_record(rec, logprobs_ref(raw, t, 2), k)
        ranks.append(rec["rank"])
    print("ranks of the penalised picks under the raw logits:", ranks)
    _check_teacher_forced(w, toks, _prompt_rows(proc, PROMPT), penalties.rows(1, 1.3, 0.5, 0.5, {EOS: -INF}))


def test_replan_after_a_failed_step_rebuilds_the_tables(monkeypatch, capsys):
    """the loop's recovery drops the captures and rewinds: the tables are rebuilt from the prompt and the tokens fed so far"""
    from phi_3_vision_mlx_amd import api, ops
    from phi_3_vision_mlx_amd.api import load_synthetic
    model, _ = load_synthetic(blind_model=True, tiny=False, seed=0, device="cuda:0", num_hidden_layers=2)
    ids = torch.randint(3, 32000, (1, 1700), dtype=torch.int64, generator=torch.Generator().manual_seed(6)).numpy()
    rows = penalties.rows(1, 1.3, 0.5, 0.5, None)

    def run(fail):
        if fail is None:
            monkeypatch.delenv("P3V_DEBUG_FAIL_STEP", raising=False)
        else:
            monkeypatch.setenv("P3V_DEBUG_FAIL_STEP", str(fail))
        model.serving = False
        logits, cache = model(input_ids=torch.as_tensor(ids), max_tokens=40)
        st = cache[0].state
        model.set_penalties(st, penalties.pack(rows), ids, 0)
        token = ops.argmax(model.penalized_logits(st, logits))[:, None]
        seen = []
        api.greedy_loop(model, token, cache, 10, lambda r: seen.append(list(r)), lambda r: False, penalties=dict(prompt_ids=ids, pad=None))
        fed = token.reshape(-1).cpu().tolist() + [r[0] for r in seen[:-1]]
        table = _u32_of(st.penalty["seen"]).reshape(-1)
        assert np.array_equal(table, penalties.seen_table(ids[0], fed, table.size))
        return seen, st.graphs["greedy"]["bufs"]["plan"].fuse_o

    good, fused = run(None)
    assert fused and len(good) == 10
    for fail in (0, 4):
        got, fused2 = run(fail)
        assert got == good and not fused2
        assert "continuing with separate launches" in capsys.readouterr().err
    del model
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------- engine
def test_engine_requests_equal_their_solo_runs_and_slots_are_handed_over_clean(tiny):
    """penalised greedy, plain, sampled + penalised and bias-only requests (and a fifth, plain) through two slots: each returns
    the tokens of its solo B = 1 api.generate run.  A draw is a function of the row's logits, so the sampled request must see
    the logits of its solo run: it is the longest prompt and submitted first (no left padding: the column of an idle engine is
    its head's length), in an engine whose window gives the cache the capacity of the solo run's (one 128-key tile: the same
    split plan).  The greedy requests are refilled, left-padded rows: their arg-max does not hang on the last bit."""
    from phi_3_vision_mlx_amd.engine import ContinuousEngine, penalty_args
    model, proc = tiny
    texts = [BATCH[1], BATCH[0], BATCH[3], BATCH[2], BATCH[0]]
    pens = [dict(repetition_penalty=1.2, presence_penalty=0.25), None,
            dict(repetition_penalty=1.3, frequency_penalty=0.5, presence_penalty=0.5), dict(logit_bias={"11": 3.0, str(EOS): -INF}), None]
    samp = [{"temperature": 0.8, "seed": 7}, None, None, None, None]
    budget = [8, 5, 6, 7, 8]
    eng = ContinuousEngine(model, proc, slots=2, window=96)
    assert eng.st.Tp == 128
    hs = []
    for i in range(5):
        inputs = proc(texts[i]) if pens[i] is None else penalty_args(proc(texts[i]), **pens[i])
        hs.append(eng.submit(inputs, budget[i], **({} if samp[i] is None else {"sampling": samp[i]})))
    eng.run_until_idle()
    assert all(h.error is None for h in hs), [h.error for h in hs]
    assert eng.failures == 0
    rows_used = [h.row for h in hs]
    assert len(set(rows_used)) == 2                                               # five requests through two slots: refilled
    pen_rows = {hs[i].row for i in (0, 2, 3)}
    assert hs[4].row in pen_rows or hs[1].row in pen_rows                         # a plain request took over a penalised row's slot
    for i in range(5):
        kw = dict(pens[i] or {})
        if samp[i]:
            kw.update(temperature=samp[i]["temperature"], seed=samp[i]["seed"])
        solo, _ = _gen(model, proc, texts[i], max_tokens=budget[i], **kw)
        want = solo[0][:solo[0].index(EOS) + 1] if EOS in solo[0] else solo[0]
        print(i, "engine", hs[i].tokens, "solo", want)
        assert hs[i].tokens == want, i
    rec = penalties.unpack(eng.st.penalty["rows"])
    assert all(r["flags"] == 0 for r in rec)                                      # every row released: inactive records
