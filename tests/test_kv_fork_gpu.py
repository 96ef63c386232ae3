"""p3v_kv_fork (n completions per prompt: one source row to many rows) -- the kernel against torch indexing, BIT-equal,
its refusals, and `model.fork_rows` / `model.fork_state` against the copy the prefix cache already had.

Kernel cases: nl = nkv = 2; hd 32 and 96; bf16 and int8 codes + fp32 scale rows; n_tok in {0, 1, 7, 8, 9, 69, 300} (300
tokens of hd 96 at 2 bytes are more than one `part` per (layer, head) unit); a shared t0 in {0, 1, 3, 8, 13} and, between two
allocations, t0_src != t0_dst at equal 16-byte phase; 1, 2, 5 and 15 destination rows, unordered and non-adjacent; rows of
ONE state (B = 16) and two allocations of different B and T.  Both sides start as distinct random patterns; the WHOLE
destination and the whole source are compared afterwards, so every byte outside the destination runs is checked."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NL, NKV = 2, 2
DEV = "cuda:0"
N_TOK = [0, 1, 7, 8, 9, 69, 300]
T0 = [0, 1, 3, 8, 13]
N_DST = [1, 2, 5, 15]
B_SRC = 5
DST_ROWS = [9, 2, 14, 0, 7, 11, 3, 15, 1, 12, 6, 13, 4, 10, 8]    # every row of 16 but B_SRC, unordered


@pytest.fixture(scope="module")
def ops():
    from phi_3_vision_mlx_amd import ops as o
    o.L.lib()
    return o


def rand_cache(B, T, hd, es, seed):
    """(k, vt) bf16 or (k8, v8t, ks, vs): random bits (compared as integers, so NaN patterns are fine)."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    if es == 2:
        return (torch.randint(-32768, 32768, (NL, B, NKV, T, hd), dtype=torch.int16, device=DEV, generator=g).view(torch.bfloat16),
                torch.randint(-32768, 32768, (NL, B, NKV, hd, T), dtype=torch.int16, device=DEV, generator=g).view(torch.bfloat16))
    return (torch.randint(0, 256, (NL, B, NKV, T, hd), dtype=torch.uint8, device=DEV, generator=g),
            torch.randint(0, 256, (NL, B, NKV, hd, T), dtype=torch.uint8, device=DEV, generator=g),
            torch.rand((NL, B, NKV, T), dtype=torch.float32, device=DEV, generator=g) + 0.5,
            -torch.rand((NL, B, NKV, T), dtype=torch.float32, device=DEV, generator=g) - 0.5)


def bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32) if t.dtype == torch.float32 else t


def same(a, b):
    return all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


def expect(dst, src, b_s, t0_s, rows, t0_d, n):
    """The fork with torch indexing (src: untouched clones of the source tensors)."""
    for b_d in rows:
        dst[0][:, b_d, :, t0_d:t0_d + n, :] = src[0][:, b_s, :, t0_s:t0_s + n, :]
        dst[1][:, b_d, :, :, t0_d:t0_d + n] = src[1][:, b_s, :, :, t0_s:t0_s + n]
        for d, s in zip(dst[2:], src[2:]):
            d[:, b_d, :, t0_d:t0_d + n] = s[:, b_s, :, t0_s:t0_s + n]


@pytest.fixture(scope="module")
def pools():
    """The random tensors of every (es, hd), made once and never written: each launch works on clones."""
    out = {}
    for es in (2, 1):
        for hd in (32, 96):
            out[es, hd] = dict(one=rand_cache(16, 384, hd, es, 11), src=rand_cache(2, 384, hd, es, 23), dst=rand_cache(16, 640, hd, es, 37))
    return out


@pytest.mark.parametrize("n", N_TOK)
@pytest.mark.parametrize("hd", [32, 96])
@pytest.mark.parametrize("es", [2, 1])
def test_fork_bit_equal_and_nothing_else_written(ops, pools, es, hd, n):
    pool = pools[es, hd]
    for t0 in T0:
        for m in N_DST:
            rows = DST_ROWS[:m]
            # rows of ONE state
            st = tuple(t.clone() for t in pool["one"])
            want = tuple(t.clone() for t in pool["one"])
            expect(want, pool["one"], B_SRC, t0, rows, t0, n)
            ops.kv_fork(st, B_SRC, t0, st, rows, t0, n)
            assert same(st, want), (es, hd, n, t0, m, "one state")
            # two allocations, B 2 -> 16 and T 384 -> 640: the shared t0, and another column of the same 16-byte phase
            for t0_d in (t0, t0 + 16 // es):
                src = tuple(t.clone() for t in pool["src"])
                dst = tuple(t.clone() for t in pool["dst"])
                want = tuple(t.clone() for t in pool["dst"])
                expect(want, pool["src"], 1, t0, rows, t0_d, n)
                ops.kv_fork(src, 1, t0, dst, rows, t0_d, n)
                assert same(dst, want), (es, hd, n, t0, t0_d, m, "two allocations")
                assert same(src, pool["src"]), (es, hd, n, t0, t0_d, m, "source written")
    torch.cuda.synchronize()


def _rec(L, src, dst, rows=(1,), **kw):
    j = L.KvFork()
    j.k_src, j.v_src, j.k_dst, j.v_dst = src[0].data_ptr(), src[1].data_ptr(), dst[0].data_ptr(), dst[1].data_ptr()
    if len(src) == 4:
        j.ks_src, j.vs_src, j.ks_dst, j.vs_dst = src[2].data_ptr(), src[3].data_ptr(), dst[2].data_ptr(), dst[3].data_ptr()
    j.B_src, j.T_src, j.B_dst, j.T_dst = src[0].shape[1], src[0].shape[3], dst[0].shape[1], dst[0].shape[3]
    j.b_src = j.t0_src = j.t0_dst = 0
    j.n_tok, j.n_dst = 8, len(rows)
    for i, b in enumerate(rows):
        j.b_dst[i] = b
    for k, v in kw.items():
        setattr(j, k, v)
    return j


def test_refusals_return_their_code_and_write_nothing(ops):
    L = ops.L
    lib = L.lib()
    src, dst = rand_cache(2, 128, 96, 2, 1), rand_cache(4, 128, 96, 2, 2)
    src8, dst8 = rand_cache(2, 128, 96, 1, 3), rand_cache(4, 128, 96, 1, 4)
    odd8 = rand_cache(2, 136, 96, 1, 5)                           # 136-byte V^T rows: not on the 16-byte grid
    keep = [tuple(t.clone() for t in c) for c in (src, dst, src8, dst8, odd8)]
    stream = torch.cuda.current_stream().cuda_stream

    def call(j, nl=NL, nkv=NKV, hd=96, es=2):
        return lib.p3v_kv_fork(ctypes.byref(j), nl, nkv, hd, es, stream)

    ok = _rec(L, src, dst)
    err_arg = [
        call(_rec(L, src, dst, k_src=0)), call(_rec(L, src, dst, v_dst=0)),                    # null pointers
        call(_rec(L, src, dst, k_dst=dst[0].data_ptr() + 2)),                                  # K base off the 16-byte grid
        call(_rec(L, src, dst, v_src=src[1].data_ptr() + 1)),                                  # bf16 V^T base at an odd byte
        call(_rec(L, src8, dst8, ks_src=src8[2].data_ptr() + 2), es=1),                        # a scale base off its 4 bytes
        call(_rec(L, src, dst, ks_src=src[0].data_ptr())),                                     # one scale pointer of four
        call(_rec(L, src, dst, n_dst=0)), call(_rec(L, src, dst, n_dst=16)), call(_rec(L, src, dst, n_dst=-1)),
        call(ok, es=4), call(ok, es=3), call(ok, es=0),
        call(ok, hd=100),                                                                      # 200-byte K rows
        call(ok, nl=0), call(ok, nkv=0), call(ok, hd=0),
        call(_rec(L, src, dst, b_src=2)), call(_rec(L, src, dst, b_src=-1)),                   # a row index outside its B
        call(_rec(L, src, dst, rows=(4,))), call(_rec(L, src, dst, rows=(0, -1))),
        call(_rec(L, src, dst, t0_src=121)), call(_rec(L, src, dst, t0_dst=121)),              # the run leaves its row: 121 + 8 > 128
        call(_rec(L, src, dst, t0_dst=-8)), call(_rec(L, src, dst, n_tok=-1)), call(_rec(L, src, dst, n_tok=129)),
        call(_rec(L, src, dst, rows=(1, 3, 1))),                                               # two equal destination rows
        call(_rec(L, dst, dst, rows=(1, 0, 2))),                                               # one state, a destination row = b_src
        call(_rec(L, (dst[0][:, 1:], dst[1][:, 1:]), dst, B_src=3)),                           # another view of the destination's memory
        call(_rec(L, (dst[0], src[1]), (dst[0][1:], dst[1]), rows=(1,))),                      # K alone shared, as a different view
        lib.p3v_kv_fork(None, NL, NKV, 96, 2, stream),
    ]
    assert err_arg == [-22] * len(err_arg), err_arg
    unsupported = [
        call(_rec(L, src, dst, t0_dst=1)), call(_rec(L, src, dst, t0_src=3, t0_dst=8)),        # unequal 16-byte phase (bf16: mod 8)
        call(_rec(L, src8, dst8, t0_src=3, t0_dst=11), es=1),                                  # ... int8: 3 and 11 differ mod 16
        call(_rec(L, odd8, dst8), es=1), call(_rec(L, src8, odd8), es=1),                      # rows off the 16-byte grid, either side
    ]
    assert unsupported == [L.ERR_UNSUPPORTED] * len(unsupported), unsupported
    torch.cuda.synchronize()
    for c, k in zip((src, dst, src8, dst8, odd8), keep):
        assert same(c, k)
    # the legal neighbours of the cases above, and the empty job
    assert call(ok) == 0 and call(_rec(L, dst, dst, rows=(1, 3, 2))) == 0 and call(_rec(L, src8, dst8, t0_src=3, t0_dst=19), es=1) == 0
    assert call(_rec(L, src, dst, n_tok=0, t0_src=128, t0_dst=128)) == 0
    assert call(_rec(L, src, dst, n_tok=0, t0_dst=1)) == 0 and call(_rec(L, odd8, dst8, n_tok=0), es=1) == 0   # ... at any phase
    assert call(_rec(L, src, dst, n_tok=0, rows=(1, 1))) == -22                  # (its arguments are still checked)
    with pytest.raises(ValueError):
        ops.kv_fork(src, 0, 0, dst, [], 0, 1)
    with pytest.raises(ValueError):
        ops.kv_fork(src, 0, 0, rand_cache(16, 128, 96, 2, 6), list(range(16)), 0, 1)
    with pytest.raises((TypeError, ValueError)):
        ops.kv_fork(src, 0, 0, dst8, [1], 0, 1)
    with pytest.raises(RuntimeError):
        ops.kv_fork(src, 0, 0, dst, [1], 1, 1)                     # phase mismatch: raised, never a silent other path
    assert ctypes.sizeof(L.KvFork) == 160
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- model level
EOS = 32007
SEED = 20240611
COL = 2560                                                        # the slot states' column: the image request has 26 columns of padding
STEPS = 6
_MEMO = {}


class IdTokenizer:
    """Delegates encoding to the real tokenizer; decodes to the ids themselves, so texts compare as tokens."""

    def __init__(self, real):
        self.real = real

    def __call__(self, *a, **kw):
        return self.real(*a, **kw)

    def encode(self, *a, **kw):
        return self.real.encode(*a, **kw)

    def decode(self, ids, **kw):
        return " ".join(str(int(i)) for i in ids)

    def batch_decode(self, seqs, **kw):
        return [self.decode(s) for s in seqs]


def _serve(kind="bf16"):
    """The tiny model of tests/golden/tiny_serve_oracle.npz (bf16 or int8 KV cache), its processor and the fixture's requests."""
    if kind not in _MEMO:
        from golden_inputs import serve_requests
        from test_model_gpu import GOLDEN
        from phi_3_vision_mlx_amd.api import load_synthetic
        g = np.load(GOLDEN + "/tiny_serve_oracle.npz")
        model, proc = load_synthetic(blind_model=False, tiny=True, seed=0, std_scale=4.0, device="cuda:0",
                                     lm_head_spread=float(g["spread"][0]), lm_head_seed=int(g["head_seed"][0]),
                                     **(dict(use_quantized_cache=True) if kind == "int8" else {}))
        reqs = serve_requests(proc)
        proc.tokenizer = IdTokenizer(proc.tokenizer)
        _MEMO[kind] = (g, model, proc, reqs)
    return _MEMO[kind]


def _cache_of(st):
    return [type("L", (), {"state": st})()]


def _kv(st):
    return (st.k8, st.v8, st.ks, st.vs) if st.quantized else (st.k, st.v)


def _bits_row(t):
    return t.detach().reshape(-1).view(torch.int16).cpu().numpy().view(np.uint16)


def _fork_runs(kind, which):
    """State A (prefill_slot into row 0 of a 4-row slot state + fork_rows to rows 1..3) and state B (the same prefill, rows 1..3
    filled by ops.kv_copy jobs and torch copies of the table rows: what the parent can do), each followed by the first draw and
    6 sampled steps under seeds s + j.  Computed once per (cache kind, request) and shared by the tests below."""
    key = ("runs", kind, which)
    if key in _MEMO:
        return _MEMO[key]
    from phi_3_vision_mlx_amd import ops, sampling
    g, model, proc, reqs = _serve(kind)
    req = reqs[0] if which == "image" else reqs[2]
    S = int(np.asarray(req["input_ids"]).shape[-1])
    recs = sampling.rows(4, 0.9, 50, 0.95, SEED)
    out = {"recs": recs, "S": S}
    for name in ("A", "B"):
        st = model.new_slot_state(4, 4096)
        st.offset = COL
        if not st.quantized:
            st.k.zero_()                                           # (torch.empty: the two states' untouched columns must compare)
        _, logits = model.prefill_slot(st, 0, req, return_logits=True)
        pad, kv = COL - S, _kv(st)
        if name == "A":
            model.fork_rows(st, 0, [1, 2, 3])
        else:
            ops.kv_copy([(kv, 0, pad, kv, r, pad, S) for r in (1, 2, 3)])
            for r in (1, 2, 3):
                st.cos[r].copy_(st.cos[0]), st.sin[r].copy_(st.sin[0]), st.pad_len[r:r + 1].copy_(st.pad_len[0:1])
        torch.cuda.synchronize()
        snap = [t.clone() for t in kv] + [st.cos.clone(), st.sin.clone(), st.pad_len.clone()]
        model.set_sampling(st, sampling.pack(recs, 0))
        token = model.sample_logits(st, logits[:, -1].expand(4, -1).contiguous())      # draw 0 of every row: the ONE prefill row
        lgs, toks = [logits[0, -1].clone()], [token.reshape(-1).tolist()]
        cache = _cache_of(st)
        for _ in range(STEPS):
            lg, token = model.sample_step(token, cache)
            torch.cuda.synchronize()
            lgs.append(lg.reshape(4, -1).clone())
            toks.append(token.reshape(-1).tolist())
        out[name] = dict(snap=snap, lgs=lgs, toks=toks, counters=[r["counter"] for r in sampling.unpack(st.sample_rows)], pad=pad)
        del st
    _MEMO[key] = out
    return out


@pytest.mark.parametrize("which", ["text", "image"])
@pytest.mark.parametrize("kind", ["bf16", "int8"])
def test_fork_rows_equals_the_copy_the_prefix_cache_had(kind, which):
    run = _fork_runs(kind, which)
    a, b = run["A"], run["B"]
    names = (["k8", "v8t", "k_scale", "v_scale"] if kind == "int8" else ["k", "vt"]) + ["cos", "sin", "pad_len"]
    for name, x, y in zip(names, a["snap"], b["snap"]):
        assert torch.equal(bits(x), bits(y)), (kind, which, name)
    # the forked rows really hold the source row's columns (and its tables): state A against itself
    pad, S = a["pad"], run["S"]
    assert a["snap"][-1].tolist() == [pad] * 4
    k, vt = bits(a["snap"][0])[:, :, :, pad:COL], bits(a["snap"][1])[..., pad:COL]        # K [nl, B, nkv, T, hd], V^T [nl, B, nkv, hd, T]
    assert all(torch.equal(k[:, r], k[:, 0]) and torch.equal(vt[:, r], vt[:, 0]) for r in (1, 2, 3)), (kind, which)
    assert bool((k[:, 0] != k[:, 0, :, :1]).any())                                        # (not all one value: the prompt is there)
    for step, (la, lb) in enumerate(zip(a["lgs"], b["lgs"])):
        assert torch.equal(bits(la), bits(lb)), (kind, which, "logits of step", step)
    assert a["toks"] == b["toks"], (kind, which)
    assert len({tuple(t[r] for t in a["toks"]) for r in range(4)}) > 1, "four seeds gave four equal rows: nothing was sampled"


@pytest.mark.parametrize("which", ["text", "image"])
@pytest.mark.parametrize("kind", ["bf16", "int8"])
def test_forked_rows_follow_the_sampling_rule(kind, which):
    """Every row's token at every step is the rule's (test_sampling_cpu.sample_ref) on that step's own logits row under the row's
    record: seed s + j, draw index = the step (draw 0 from the prefill row); the counters end at steps + 1."""
    from test_sampling_cpu import sample_ref
    run = _fork_runs(kind, which)
    a, recs = run["A"], run["recs"]
    assert [r[3] for r in recs] == [SEED + j for j in range(4)]
    first = _bits_row(a["lgs"][0])
    assert a["toks"][0] == [sample_ref(first, *recs[j], 0) for j in range(4)]
    for step in range(1, STEPS + 1):
        want = [sample_ref(_bits_row(a["lgs"][step][j]), *recs[j], step) for j in range(4)]
        assert a["toks"][step] == want, (kind, which, step)
    assert a["counters"] == [STEPS + 1] * 4


def test_greedy_family_of_three_matches_the_oracle():
    """api._generate(n=3) at temperature 0: three equal completions, equal to the fixture's tokens up to the request's first
    unclear step (the fixtures' own clearance rule), for the image request and a text request."""
    from golden_inputs import SERVE_STEPS, SERVE_TEXTS, make_image
    from test_serving_gpu import tokens_vs_fixture
    from phi_3_vision_mlx_amd import api
    g, model, proc, _ = _serve()
    for i, imgs in ((0, [make_image(336, 336, "noise", 0)]), (2, None)):
        forks = []
        real = model.fork_state
        model.fork_state = lambda st, n: forks.append((st.B, st.offset, n)) or real(st, n)
        try:
            out = api._generate(model, proc, SERVE_TEXTS[i], imgs, max_tokens=SERVE_STEPS, verbose=False, stream=False, mute=True, n=3)
        finally:
            del model.fork_state
        assert isinstance(out, list) and len(out) == 3 and forks == [(1, int(g["n_ids"][i]), 3)]      # ONE prefill, forked once
        toks = [[int(t) for t in s.split()] for s in out]
        assert toks[0] == toks[1] == toks[2]
        n = tokens_vs_fixture([toks[0]], g, f"greedy family, request {i}", rows=[i], min_first=1)
        assert n >= 1
        print(f"request {i}: {n} tokens of each of 3 completions equal the oracle's")


# ---------------------------------------------------------------------------------------------------- engine
def _hand_family(model, slots, col, rows, req, recs, n_steps, pen=None, want=None, adapter=None):
    """The rows of a family driven by hand through the existing setters: records first, prefill_slot into rows[0], fork_rows,
    the first tokens from the one logits row, then n_steps captured steps.  -> ({row: tokens}, {row: records})."""
    from phi_3_vision_mlx_amd import logprobs as lpm, penalties as pm, sampling
    st = model.new_slot_state(slots, 4096)
    st.serving = True                                              # (as the engine's state: the same split-KV plan)
    st.offset = col
    g = model.decode_graph(st)
    if adapter is not None:
        for r in rows:
            model.set_row_adapters(st, [adapter], r)
    if pen is not None:
        ids2 = np.asarray(req["input_ids"]).reshape(1, -1)
        for r in rows:
            model.set_penalties(st, pm.pack([pen]), ids2, r, bias=pm.bias_table([pen], model.cfg.vocab_size))
    for r, rec in zip(rows, recs):
        model.set_sampling(st, sampling.pack([rec], 0), r)
    _, logits = model.prefill_slot(st, rows[0], req, return_logits=True)
    model.fork_rows(st, rows[0], rows[1:])
    toks, records = {r: [] for r in rows}, {r: [] for r in rows}
    for r in rows:
        t = model.sample_logits(st, model.penalized_logits(st, logits, r) if pen is not None else logits, r)
        g["tok"][r:r + 1].copy_(t.reshape(-1))
        toks[r].append(int(t))
        if want is not None:
            model.set_logprobs(st, [want], r)
            records[r].append(lpm.unpack(model.logprobs_of(st, logits, t.reshape(1), r))[0])
    step = {(False, False): model.sample_step, (True, False): model.penal_step, (False, True): model.sample_logprob_step,
            (True, True): model.penal_logprob_step}[(pen is not None, want is not None)]
    cache = _cache_of(st)
    for _ in range(n_steps):
        _, tok = step(g["host_tok"] if g["host_tok"] is not None else g["tok"].view(-1, 1), cache)
        out = tok.reshape(-1).tolist()
        recs_ = lpm.unpack(g["records"][:, g["n_replays"] - 1]) if want is not None else None
        for r in rows:
            toks[r].append(out[r])
            if want is not None:
                records[r].append(recs_[r])
    return toks, records


def _cut(toks, budget):
    toks = toks[:budget]
    return toks[:toks.index(EOS) + 1] if EOS in toks else toks


def _spy_forks(model):
    calls, real = [], model.fork_rows

    def spy(st, src_row, dst_rows, pad=None):
        calls.append((int(st.offset), int(src_row), [int(r) for r in dst_rows]))
        return real(st, src_row, dst_rows, pad=pad)
    model.fork_rows = spy
    return calls


def test_engine_family_joins_mid_flight_and_equals_the_hand_driven_rows():
    """A sampled family of 3 joins a 6-slot engine while another request is generating: that request's tokens are those of a
    run without the family; the family's tokens are those of the same rows driven by hand (prefill_slot + fork_rows + captured
    steps); the completions end at different lengths (a logit_bias gives EOS a chance of about a quarter per step) and their rows
    serve later requests."""
    from test_serving_gpu import tokens_vs_fixture
    from phi_3_vision_mlx_amd import penalties as pm, sampling
    from phi_3_vision_mlx_amd.engine import ContinuousEngine, n_args, penalty_args
    g, model, proc, reqs = _serve()
    T, budget = 1.0, 12
    # a bias that puts EOS at p = 0.25 of the prompt's own first-token distribution (any value serves the comparison; this
    # one makes the completions end at different steps)
    lg = model(**reqs[3], max_tokens=1)[0][0, -1].float()
    others = torch.logsumexp(torch.cat([lg[:EOS], lg[EOS + 1:]]) / T, 0)
    bias = {EOS: float(T * (np.log(0.25 / 0.75) + others) - lg[EOS])}
    settings = dict(temperature=T, top_k=0, top_p=1.0, seed=SEED)

    def run(with_family):
        eng = ContinuousEngine(model, proc, slots=6, window=4096)
        a = eng.submit(reqs[2], 14)
        eng.step(), eng.step()
        heads = []
        if with_family:
            # two families behind each other: a plain sampled one (it runs its whole budget unless it draws EOS), and one whose
            # bias ends its rows early.  One row is busy and the first takes three: the second waits for three free rows
            heads = [eng.submit(n_args(reqs[3], 3), budget, sampling=settings),
                     eng.submit(n_args(penalty_args(reqs[3], logit_bias=bias), 3), budget, sampling=dict(settings, seed=SEED + 100))]
            eng.step()
            assert all(c.row is not None for c in heads[0].members) and all(c.row is None for c in heads[1].members)
        eng.run_until_idle()
        assert eng.failures == 0 and a.error is None
        return eng, a, heads
    _, alone, _ = run(False)
    calls = _spy_forks(model)
    try:
        eng, a, heads = run(True)
    finally:
        del model.fork_rows
    assert a.tokens == alone.tokens and len(a.tokens) >= 3                       # the running request never noticed
    assert len(calls) == 2 and eng.joined_mid_flight >= 3
    used = set()
    for head, (col, src, dst), seed, pen in zip(heads, calls, (SEED, SEED + 100),
                                                (None, pm.request_row(dict(logit_bias=bias), model.cfg.vocab_size))):
        assert head.family_done.is_set() and len(head.completions) == 3 and head.completions[0] is head
        assert all(c.error is None and c.done.is_set() for c in head.completions)
        rows = [src] + dst
        assert rows == [c.row for c in head.members] and len(set(rows)) == 3
        recs = [(T, 0, 1.0, seed + j) for j in range(3)]
        assert [c.sampling for c in head.members] == recs
        toks, _ = _hand_family(model, 6, col, rows, reqs[3], recs, budget - 1, pen=pen)
        for c in head.members:
            assert c.tokens == _cut(toks[c.row], budget), (c.row, c.tokens, toks[c.row])
        print("family lengths:", [len(c.tokens) for c in head.members], "rows", rows, "column", col)
        used |= set(rows)
    assert a.row not in [c.row for c in heads[0].members]
    assert max(len(c.tokens) for c in heads[0].members) >= 6                     # the comparison above covered real decode steps
    lens = [len(c.tokens) for c in heads[1].members]
    assert len(set(lens)) > 1, lens                                               # completions leave at their own EOS
    rows = sorted(used)
    # the family's rows serve later requests (greedy, unpenalised: the rows' records were reset), which match the oracle
    later = [eng.submit(reqs[i], 6) for i in (1, 2, 3, 4, 5, 6)]
    eng.run_until_idle()
    assert all(h.error is None for h in later) and set(rows) <= {h.row for h in later}
    assert tokens_vs_fixture([h.tokens for h in later], g, "rows reused after a family", rows=[1, 2, 3, 4, 5, 6], min_first=1, budgets=[6] * 6) >= 6


def test_engine_best_of_returns_the_ranking_functions_choice():
    from phi_3_vision_mlx_amd.engine import ContinuousEngine, n_args
    from phi_3_vision_mlx_amd.logprobs import cumulative, rank_best_of
    g, model, proc, reqs = _serve()
    eng = ContinuousEngine(model, proc, slots=6, window=4096)
    head = eng.submit(n_args(reqs[3], 3, 5), 8, sampling=dict(temperature=1.0, seed=SEED))
    assert head.completions is None
    eng.run_until_idle()
    assert head.family_done.is_set() and len(head.members) == 5 and all(c.error is None for c in head.members)
    assert all(len(c.logprob_records) == len(c.tokens) and [r["token"] for r in c.logprob_records] == c.tokens for c in head.members)
    ids, lps = [c.tokens for c in head.members], [[r["logprob"] for r in c.logprob_records] for c in head.members]
    order = rank_best_of(ids, lps, 3, EOS)
    assert head.completions == [head.members[j] for j in order]
    scores = [cumulative(i, l, EOS) for i, l in zip(ids, lps)]
    assert all(np.isfinite(scores)) and min(scores[j] for j in order) >= max([scores[j] for j in range(5) if j not in order])
    assert [scores[j] for j in order] == sorted((scores[j] for j in order), reverse=True)
    assert len({c.sampling[3] for c in head.members}) == 5 and head.asked_logprobs is None
    print("best_of scores:", [round(s, 3) for s in scores], "returned:", order)


def test_family_with_penalties_logprobs_and_an_adapter_equals_the_hand_driven_rows():
    from gen_golden_adapters import fixture_adapter
    from phi_3_vision_mlx_amd import penalties as pm
    from phi_3_vision_mlx_amd.api import load_synthetic
    from phi_3_vision_mlx_amd.engine import ContinuousEngine, logprob_args, n_args, penalty_args
    from phi_3_vision_mlx_amd.weights import resolve_adapter
    model, proc = load_synthetic(blind_model=True, tiny=True, seed=0, std_scale=4.0, device="cuda:0")
    model.set_adapter_bank({n: resolve_adapter(model.cfg, *fixture_adapter(model.cfg, n)) for n in ("A", "B")})
    req = proc("<|user|>\nTell me a story about a story about a story<|end|>\n<|assistant|>\n")
    S, budget = int(np.asarray(req["input_ids"]).shape[-1]), 9
    pd = dict(repetition_penalty=1.3, presence_penalty=0.4, frequency_penalty=0.2, logit_bias={17: -float("inf"), 29: 1.5})
    eng = ContinuousEngine(model, proc, slots=4, window=4096)
    calls = _spy_forks(model)
    try:
        head = eng.submit(n_args(logprob_args(penalty_args(req, **pd), 2), 3), budget, sampling=dict(temperature=0.8, top_k=40, seed=SEED),
                          adapter="A")
        eng.run_until_idle()
    finally:
        del model.fork_rows
    assert head.family_done.is_set() and all(c.error is None for c in head.completions) and eng.failures == 0
    assert calls == [(S, 0, [1, 2])]
    recs = [(0.8, 40, 1.0, SEED + j) for j in range(3)]
    toks, records = _hand_family(model, 4, S, [0, 1, 2], req, recs, budget - 1, pen=pm.request_row(pd, model.cfg.vocab_size), want=2,
                                 adapter="A")
    for c in head.completions:
        want = _cut(toks[c.row], budget)
        assert c.tokens == want and c.logprob_records == records[c.row][:len(want)], (c.row, c.tokens, want)
        assert all(len(r["top"]) == 2 for r in c.logprob_records) and 17 not in c.tokens
    assert len({tuple(c.tokens) for c in head.completions}) > 1
    # the adapter is part of it: the same family on the base model reads other logits
    base = eng.submit(n_args(logprob_args(penalty_args(req, **pd), 2), 3), budget, sampling=dict(temperature=0.8, top_k=40, seed=SEED))
    eng.run_until_idle()
    assert [c.logprob_records[0]["logprob"] for c in base.completions] != [c.logprob_records[0]["logprob"] for c in head.completions]


# ---------------------------------------------------------------------------------------------------- n == 1, HTTP
class _Count:
    """Counts the library's launches by name (everything but the graph / event helpers and the queries)."""

    def __init__(self):
        from phi_3_vision_mlx_amd import _lib
        self._lib, self.real, self.n = _lib, _lib.lib(), {}

    def __getattr__(self, name):
        fn = getattr(self.real, name)
        if not name.startswith("p3v_") or name.startswith(("p3v_graph", "p3v_event", "p3v_device", "p3v_get", "p3v_set", "p3v_str",
                                                            "p3v_version")) or name.endswith(("_bytes", "_slices", "_role", "_can_fuse_oproj")):
            return fn

        def counted(*a):
            self.n[name] = self.n.get(name, 0) + 1
            return fn(*a)
        return counted

    def __enter__(self):
        self._lib._lib = self
        return self

    def __exit__(self, *a):
        self._lib._lib = self.real


def test_n_1_is_the_plain_path_launch_for_launch(monkeypatch):
    from golden_inputs import SERVE_TEXTS
    from phi_3_vision_mlx_amd import api, ops
    g, model, proc, _ = _serve()
    text, n_tok = SERVE_TEXTS[2], 8
    monkeypatch.setenv("P3V_PREFILL_GRAPH", "0")                  # (every run below prefills eagerly: comparable launch counts)

    def plain():
        logits, cache = model(**proc(text), max_tokens=n_tok)
        tok = ops.argmax(logits[:, -1, :].contiguous())[:, None]
        first = int(tok[0, 0])
        for _ in range(n_tok - 1):
            _, tok = model.greedy_step(tok, cache)
        torch.cuda.synchronize()
        gph = cache[0].state.graphs["greedy"]
        return [first] + gph["history"][0, :n_tok - 1].tolist(), sorted(cache[0].state.graphs)

    def via_generate(**kw):
        states, real = [], model._new_state

        def spy(*a, **k):
            states.append(real(*a, **k))
            return states[-1]
        model._new_state = spy
        try:
            out = api._generate(model, proc, text, max_tokens=n_tok, verbose=False, stream=False, mute=True, **kw)
        finally:
            del model._new_state
        return out, [(s.B, sorted(s.graphs)) for s in states]
    plain()                                                       # (uncounted: builds what a model builds once)
    with _Count() as c_plain:
        toks_p, graphs_p = plain()
    with _Count() as c_default:
        out_d, states_d = via_generate()
    with _Count() as c_n1:
        out_1, states_1 = via_generate(n=1)
    with _Count() as c_b1:
        out_b, states_b = via_generate(n=1, best_of=1)
    with _Count() as c_n3:
        out_3, states_3 = via_generate(n=3)
    assert c_default.n == c_n1.n == c_b1.n, (c_default.n, c_n1.n, c_b1.n)
    drop = lambda d: {k: v for k, v in d.items() if k != "p3v_argmax"}       # (the host loop's own token plumbing)
    assert drop(c_n1.n) == drop(c_plain.n), (c_n1.n, c_plain.n)
    assert "p3v_kv_fork" not in c_n1.n and states_d == states_1 == states_b == [(1, graphs_p)]
    assert out_d == out_1 == out_b and len(out_1) == 1 and [int(t) for t in out_1[0].split()] == toks_p[:len(out_1[0].split())]
    # and the family: exactly one fork launch on top, one prefill state and no other new one from model._new_state
    # (its first token is the single request's: the same prefill row; later ones come from the B = 3 step)
    assert c_n3.n["p3v_kv_fork"] == 1 and len(states_3) == 1 and states_3[0][0] == 1
    assert len(out_3) == 3 and out_3[0] == out_3[1] == out_3[2] and out_3[0].split()[0] == out_1[0].split()[0]


def test_http_n_3_returns_three_seeds_and_each_reproduces_alone():
    import json
    import threading
    import urllib.request
    from phi_3_vision_mlx_amd.api import load_synthetic
    from phi_3_vision_mlx_amd.engine import ContinuousEngine
    from phi_3_vision_mlx_amd.server import serve_continuous
    model, proc = load_synthetic(blind_model=True, tiny=True, seed=0, std_scale=4.0, device="cuda:0")
    httpd, backend = serve_continuous(ContinuousEngine(model, proc, slots=4, window=4096), port=0)
    threading.Thread(target=httpd.serve_forever, daemon=True).start()
    port = httpd.server_address[1]

    def post(body):
        r = urllib.request.Request(f"http://127.0.0.1:{port}/v1/completions", data=json.dumps(body).encode(),
                                   headers={"Content-Type": "application/json"})
        with urllib.request.urlopen(r, timeout=300) as resp:
            return json.loads(resp.read())
    try:
        body = {"prompt": "Once upon a time", "max_tokens": 12, "temperature": 1.0, "top_p": 0.9}
        a = post({**body, "seed": 42, "n": 3})
        assert set(a) == {"model", "responses", "seeds"} and len(a["responses"]) == 3 and a["seeds"] == [42, 43, 44]
        assert len(set(a["responses"])) > 1
        for j, s in enumerate(a["seeds"]):
            alone = post({**body, "seed": s, "n": 1})
            assert alone == {"model": "phi-3-vision", "responses": [a["responses"][j]], "seeds": [s]}, j
            assert post({**body, "seed": s}) == alone                         # without "n": the same bytes
        b = post({**body, "n": 2, "best_of": 4, "seed": 7, "logprobs": 0})
        assert len(b["responses"]) == 2 and len(b["seeds"]) == 2 and set(b["seeds"]) <= {7, 8, 9, 10} and len(b["logprobs"]) == 2
        sums = [sum(o["token_logprobs"]) for o in b["logprobs"]]
        assert sums[0] >= sums[1]                                             # best first
    finally:
        httpd.shutdown()
        backend.close()


# ---------------------------------------------------------------------------------------------------- families and the prefix store
IMG_P = 2513                       # tokens of the image request's store entry: through its last image slot


class _Spy:
    """Counts vision-tower runs and records the number of ids every decoder-stack call saw."""

    def __init__(self, model):
        self.model, self.clip, self.L = model, 0, []
        real_layers, real_clip = model._layers, model.clip_forward

        def layers(x, st, B, L, *a, **kw):
            self.L.append(B * L)
            return real_layers(x, st, B, L, *a, **kw)

        def clip(pix):
            self.clip += 1
            return real_clip(pix)
        model._layers, model.clip_forward = layers, clip

    def close(self):
        del self.model._layers, self.model.clip_forward


def test_image_family_through_the_prefix_store_hits_on_the_second_call():
    """api._generate(prompt, images, n=3, prefix_cache=store): the first call misses and leaves ONE entry under the picture's
    digest; the second restores the prompt through its last image slot (no vision tower, the prefill sees the rest of the ids
    only), leaves no further entry, and still matches the oracle; a single request of the same picture hits the family's entry."""
    from golden_inputs import SERVE_STEPS, SERVE_TEXTS, make_image
    from test_serving_gpu import tokens_vs_fixture
    from phi_3_vision_mlx_amd import api
    from phi_3_vision_mlx_amd.prefix import PrefixCache
    g, model, proc, _ = _serve()
    S = int(g["n_ids"][0])
    store = PrefixCache(1 << 30, min_tokens=64)

    def call(**kw):
        spy = _Spy(model)
        try:
            out = api._generate(model, proc, SERVE_TEXTS[0], [make_image(336, 336, "noise", 0)], max_tokens=SERVE_STEPS, verbose=False,
                                stream=False, mute=True, prefix_cache=store, **kw)
        finally:
            spy.close()
        return [[int(t) for t in s.split()] for s in out], spy
    cold, spy = call(n=3)
    c = store.counters()
    assert (c["hits"], c["misses"], c["entries"], c["bypassed"]) == (0, 1, 1, 0), c
    assert spy.clip == 1 and spy.L[0] == S
    warm, spy = call(n=3)
    c = store.counters()
    assert (c["hits"], c["misses"], c["entries"], c["tokens_reused"]) == (1, 1, 1, IMG_P), c     # a hit, and no second entry
    assert spy.clip == 0 and spy.L[0] == S - IMG_P                                   # the picture was not computed again
    assert len(warm) == 3 and warm[0] == warm[1] == warm[2] and len(cold) == 3 and cold[0] == cold[1] == cold[2]
    assert tokens_vs_fixture([cold[0]], g, "cold family through the store", rows=[0], min_first=1) >= 1
    assert tokens_vs_fixture([warm[0]], g, "warm family through the store", rows=[0], min_first=1) >= 1
    single, spy = call()
    c = store.counters()
    assert (c["hits"], c["entries"]) == (2, 1) and spy.clip == 0 and len(single) == 1
    # another picture under the same ids: a miss, never the first picture's K/V
    spy = _Spy(model)
    try:
        api._generate(model, proc, SERVE_TEXTS[0], [make_image(336, 336, "noise", 5)], max_tokens=2, verbose=False, stream=False, mute=True,
                      prefix_cache=store, n=2)
    finally:
        spy.close()
    c = store.counters()
    assert (c["hits"], c["misses"], c["entries"]) == (2, 2, 2) and spy.clip == 1


def test_engine_family_prefill_takes_a_prefix_hit():
    """The engine's family prefill with a store: the first family captures its prompt, the second is prefilled from the entry
    (cached_tokens on the head, the vision tower idle) and forked; its greedy completions match the oracle."""
    from test_serving_gpu import tokens_vs_fixture
    from golden_inputs import SERVE_STEPS, make_image
    from phi_3_vision_mlx_amd.engine import ContinuousEngine, cache_args, n_args
    from phi_3_vision_mlx_amd.prefix import PrefixCache, image_digests
    g, model, proc, reqs = _serve()
    store = PrefixCache(1 << 30, min_tokens=64)
    eng = ContinuousEngine(model, proc, slots=4, window=4096, prefix_cache=store)
    inputs = n_args(cache_args(reqs[0], image_digests=image_digests([make_image(336, 336, "noise", 0)])), 3)
    heads = []
    for _ in range(2):
        spy = _Spy(model)
        try:
            heads.append(eng.submit(inputs, SERVE_STEPS))
            eng.run_until_idle()
        finally:
            spy.close()
        if len(heads) == 1:
            assert spy.clip == 1 and int(g["n_ids"][0]) in spy.L
        else:                                                     # the picture was not computed again: the rest of the ids only
            assert spy.clip == 0 and int(g["n_ids"][0]) - IMG_P in spy.L and int(g["n_ids"][0]) not in spy.L
    cold, warm = heads
    assert cold.family_done.is_set() and warm.family_done.is_set() and eng.failures == 0
    assert all(c.error is None for c in cold.completions + warm.completions)
    assert cold.cached_tokens == 0 and warm.cached_tokens == IMG_P
    c = store.counters()
    assert (c["hits"], c["misses"], c["entries"]) == (1, 1, 1), c
    for head, what in ((cold, "cold engine family"), (warm, "warm engine family")):
        toks = [c.tokens for c in head.completions]
        assert toks[0] == toks[1] == toks[2]
        assert tokens_vs_fixture([toks[0]], g, what, rows=[0], min_first=1, budgets=[SERVE_STEPS]) >= 1
