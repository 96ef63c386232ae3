"""n completions per prompt on the host: argument checks and every refusal text, the seed rule (wrap-around at 2^64), the
best_of ranking (ties, EOS cut, -inf), the server's parsing over a stub backend, engine admission of a family over a fake
model that records `fork_rows` calls, and the fleet / router keeping a family on one engine.  The device side -- the fork
kernel, model.fork_rows / fork_state, the real engine -- is tests/test_kv_fork_gpu.py."""
import inspect
import json
import math
import os
import threading
import urllib.error
import urllib.request

import numpy as np
import pytest
import torch

from test_engine_cpu import EOS, SlotStub, req

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------- arguments, refusals, the surface
def test_surface():
    import phi_3_vision_mlx_amd as pkg
    from phi_3_vision_mlx_amd import _lib, api, engine, fleet, parallel, server
    for fn in (api.generate, api._generate):
        p = inspect.signature(fn).parameters
        assert p["n"].default == 1 and p["best_of"].default is None
    assert "n" not in inspect.signature(pkg.generate).parameters and "best_of" not in inspect.signature(pkg.generate).parameters
    for fn in (engine.ContinuousEngine.submit, engine.RegimeRouter.submit, fleet.EngineFleet.submit):
        assert list(inspect.signature(fn).parameters) == ["self", "inputs", "max_tokens", "sampling", "adapter"]   # n rides in the inputs
    for fn in (engine.ContinuousEngine.generate, engine.RegimeRouter.generate, fleet.EngineFleet.generate, server.ContinuousBackend.submit,
               server.EngineQueue.submit):
        p = inspect.signature(fn).parameters
        assert p["n"].default is None and p["best_of"].default is None
    h = open(os.path.join(ROOT, "include", "p3v.h")).read()
    assert f"#define P3V_KV_FORK_MAX_DST {_lib.KV_FORK_MAX_DST}\n" in h and parallel.MAX_N == _lib.KV_FORK_MAX_DST + 1 == 16
    import re
    body = h[h.rindex("typedef struct {", 0, h.index("} p3v_kv_fork_t")):h.index("} p3v_kv_fork_t")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for n in re.findall(r"\b(\w+)\s*(?:\[\w+\])?\s*[;,]", body)]
    assert names == [f for f, _ in _lib.KvFork._fields_]
    assert "p3v_kv_fork" in _lib.SIGNATURES and hasattr(_lib.lib(), "p3v_kv_fork")
    inputs = {"input_ids": np.zeros((1, 4), dtype=np.int64)}
    tagged = engine.n_args(inputs, 3, 5)
    assert engine.requested_n(tagged) == {"n": 3, "best_of": 5} and engine.N_ARGS not in inputs and engine.requested_n(inputs) is None


def test_check_values_and_texts():
    from phi_3_vision_mlx_amd.parallel import check
    assert check() == (1, 1) and check(1, None) == (1, 1) and check(3) == (3, 3) and check(3, 5) == (3, 5) and check(16, 16) == (16, 16)
    assert check(None, 4) == (1, 4) and check(np.int64(2)) == (2, 2)
    for bad in (0, 17, -1):
        with pytest.raises(ValueError, match=r"n must be an integer in 1\.\.16"):
            check(bad)
    for bad in (2.0, "2", True, [2]):
        with pytest.raises(ValueError, match=r"n must be an integer in 1\.\.16, got"):
            check(bad)
    for n, bad in ((3, 2), (1, 0), (2, 17)):
        with pytest.raises(ValueError, match=r"best_of must be an integer in n\.\.16"):
            check(n, bad)
    for bad in (4.0, "4", False):
        with pytest.raises(ValueError, match=r"best_of must be an integer in 1\.\.16, got"):
            check(2, bad)


class NoModel:
    """Nothing may be asked of the model (or the processor) before the arguments are refused."""

    def __getattr__(self, name):
        raise AssertionError(f"the model must not be touched ({name})")


def test_generate_refuses_before_anything_runs():
    from types import SimpleNamespace
    from phi_3_vision_mlx_amd import api, dist
    for kw, word in ((dict(n=0), "1..16"), (dict(n=17), "1..16"), (dict(n=2.5), "integer"), (dict(n=True), "integer"),
                     (dict(n=3, best_of=2), "n..16"), (dict(n=1, best_of=17), "n..16"), (dict(best_of="3"), "integer")):
        for fn, args in ((api._generate, (NoModel(), NoModel(), "hi")), (api.generate, ("hi",))):
            with pytest.raises(ValueError, match=word):
                fn(*args, **kw, **({"preload": (NoModel(), NoModel())} if fn is api.generate else {}))
    device = dict(fork_state=lambda *a: None, sample_step=lambda *a: None)
    plain = SimpleNamespace(cfg=SimpleNamespace(use_quantized_cache=False), **device)
    mlx4 = SimpleNamespace(cfg=SimpleNamespace(use_quantized_cache=True, cache_format="mlx4"), **device)
    eager = SimpleNamespace(cfg=SimpleNamespace(use_quantized_cache=False))
    with pytest.raises(ValueError, match="one prompt"):
        api._generate(plain, NoModel(), ["a", "b"], n=2)
    with pytest.raises(ValueError, match="one prompt"):
        api._generate(plain, NoModel(), ["a"], best_of=2)
    with pytest.raises(ValueError, match="speculative decoding"):
        api._generate(plain, NoModel(), "a", n=2, speculate=4)
    with pytest.raises(ValueError, match="mlx4"):
        api._generate(mlx4, NoModel(), "a", n=2)
    with pytest.raises(ValueError, match="captured step"):
        api._generate(eager, NoModel(), "a", n=2)
    with pytest.raises(ValueError, match="one adapter name"):
        api._generate(plain, NoModel(), "a", n=2, adapter=["A", "B"])
    with pytest.raises(ValueError, match="2 values for 3 rows"):
        api._generate(plain, NoModel(), "a", n=3, temperature=[0.5, 0.6])       # per-completion lists: one value per generated row
    with pytest.raises(ValueError, match="batch-sharded"):
        dist.generate_sharded(["a", "b"], preload=(NoModel(), NoModel()), n=2)
    with pytest.raises(ValueError, match="n must be"):
        dist.generate_sharded(["a"], preload=(NoModel(), NoModel()), n=0)


# ----------------------------------------------------------------------------- seeds
def test_seed_rule_and_wrap_around():
    from phi_3_vision_mlx_amd import parallel, sampling
    from phi_3_vision_mlx_amd.engine import Request, make_family
    top = (1 << 64) - 1
    assert parallel.seeds(7, 4) == [7, 8, 9, 10]
    assert parallel.seeds(top, 3) == [top, 0, 1] and parallel.seeds(top - 1, 4) == [top - 1, top, 0, 1]
    assert [r[3] for r in sampling.rows(3, 0.7, 0, 1.0, top)] == [top, 0, 1]                 # the batch rule api._generate uses for a family
    assert [r[3] for r in sampling.rows(3, 0.7, 0, 1.0, [5, 5, 9])] == [5, 5, 9]             # a list of n seeds: as given
    head = make_family(Request({"input_ids": np.zeros((1, 4), dtype=np.int64)}, 8, sampling=(0.7, 40, 0.9, top)), 3, 3)
    assert [m.sampling for m in head.members] == [(0.7, 40, 0.9, top), (0.7, 40, 0.9, 0), (0.7, 40, 0.9, 1)]
    assert head.completions == head.members and head.members[0] is head and all(m.family is head for m in head.members)
    greedy = make_family(Request({"input_ids": np.zeros((1, 4), dtype=np.int64)}, 8), 2, 4)
    assert [m.sampling for m in greedy.members] == [None] * 4 and greedy.completions is None
    assert [m.logprobs for m in greedy.members] == [0] * 4 and greedy.asked_logprobs is None  # best_of scores every member


# ----------------------------------------------------------------------------- ranking
def test_rank_best_of():
    from phi_3_vision_mlx_amd.logprobs import cumulative, rank_best_of
    inf = math.inf
    ids = [[5, 6, 7], [5, 6, 7], [5, EOS, 9], [8], [5, 6]]
    lps = [[-1.0, -1.0, -1.0], [-0.5, -0.5, -2.0], [-0.25, -0.25, -100.0], [-0.75], [-1.0, -inf]]
    assert [cumulative(i, l, EOS) for i, l in zip(ids, lps)] == [-3.0, -3.0, -0.5, -0.75, -inf]
    assert rank_best_of(ids, lps, 5, EOS) == [2, 3, 0, 1, 4]      # the EOS cut drops the -100; the tie 0 / 1 goes to the lower index
    assert rank_best_of(ids, lps, 1, EOS) == [2] and rank_best_of(ids, lps, 3, EOS) == [2, 3, 0]
    assert rank_best_of(ids, lps, 3, None) == [3, 0, 1]           # without an EOS id nothing is cut: row 2 pays its -100
    assert rank_best_of([[1], [1], [1]], [[-2.0], [-2.0], [-2.0]], 2) == [0, 1]
    assert rank_best_of([[1], None, [1, 2], []], [[-inf], None, [-1.0, float("nan")], []], 4) == [0, 1, 2, 3]   # all -inf: index order
    assert rank_best_of([[1], [2]], [[-inf], [-5.0]], 1) == [1]
    assert cumulative([1, 2], [-1.0], None) == -inf               # fewer records than tokens: not a score
    for bad in (0, 3):
        with pytest.raises(ValueError):
            rank_best_of([[1], [2]], [[-1.0], [-1.0]], bad)


# ----------------------------------------------------------------------------- engine: a fake model that records fork_rows
class ForkStub(SlotStub):
    """SlotStub plus the family interface: fork_rows copies the source row's key (its tokens are then the source's), each
    row's tokens are offset by its sampling seed so that members differ, and every call is recorded."""

    def __init__(self):
        super().__init__()
        self.forks, self.sampling_rows, self.fail_fork = [], {}, False

    def new_slot_state(self, slots, window):
        st = super().new_slot_state(slots, window)
        st.seed = np.zeros(slots, dtype=np.int64)
        return st

    def _tok(self, st):
        k = st.key + st.seed * 13                                 # (seed 0, a greedy row: SlotStub's own rule)
        t = (k * 31 + st.step * 7919) % 31000 + 3
        return np.where((k + st.step) % 29 == 28, EOS, t)

    def set_sampling(self, st, records, row0=0):
        from phi_3_vision_mlx_amd.sampling import unpack
        st.sample_rows = True                                     # (the engine resets a row's record once the state has records)
        for i, r in enumerate(unpack(records)):
            st.seed[row0 + i] = r["seed"] % 1000 if r["temperature"] > 0 else 0
            self.sampling_rows[row0 + i] = r

    def prefill_slot(self, st, row, inputs, return_logits=False):
        tok = super().prefill_slot(st, row, inputs)
        return (tok, torch.zeros((tok.shape[0], 1, 8))) if return_logits else tok

    def sample_logits(self, st, logits, row0=0):
        return torch.as_tensor(self._tok(st)[row0:row0 + 1, None].astype(np.int32))

    def fork_rows(self, st, src_row, dst_rows, pad=None):
        if self.fail_fork:
            raise RuntimeError("fork failed")
        self.forks.append((int(src_row), [int(r) for r in dst_rows], int(st.offset), pad))
        for r in dst_rows:
            st.key[r], st.step[r], st.pad_len[r] = st.key[src_row], st.step[src_row], st.pad_len[src_row]

    def sample_step(self, token, cache):
        return self.greedy_step(token, cache)

    # log-probability records (best_of ranks on them): a token's "log-probability" is a function of the token alone
    @staticmethod
    def _records(tokens):
        rec = np.zeros((len(tokens), 20), dtype=np.int32)
        rec[:, 0] = tokens
        rec[:, 1] = (-(np.asarray(tokens) % 7) / 4.0).astype(np.float32).view(np.int32)
        return torch.from_numpy(rec)

    def set_logprobs(self, st, wants, row0=0):
        st.logprob_want = True

    def logprobs_of(self, st, logits, tokens, row0=0):
        return self._records(tokens.reshape(-1).tolist())

    def logprob_step(self, token, cache):
        out = self.greedy_step(token, cache)
        g = self.decode_graph(cache[0].state)
        if "records" not in g:
            g["records"] = torch.zeros((len(g["tok"]), 64, 20), dtype=torch.int32)
        g["n_replays"] = g.get("n_replays", 0) + 1
        g["records"][:, g["n_replays"] - 1] = self._records(out[1].reshape(-1).tolist())
        return out

    sample_logprob_step = logprob_step

    def decode_graph(self, st):
        g = super().decode_graph(st)
        g.setdefault("history", torch.zeros((len(st.pad_len), 64), dtype=torch.int32))
        return g

    def restart_history(self, st):
        self.decode_graph(st)["n_replays"] = 0


def _engine(slots=4, **kw):
    from phi_3_vision_mlx_amd.engine import ContinuousEngine
    m = ForkStub()
    return m, ContinuousEngine(m, None, slots=slots, window=4096, **kw)


def test_family_is_prefilled_once_forked_and_members_leave_independently():
    from phi_3_vision_mlx_amd.engine import n_args
    m, e = _engine(4)
    head = e.submit(n_args(req(20, 1), 3), 30, sampling={"temperature": 0.8, "seed": 41})
    assert not head.done.is_set() and len(head.members) == 3 and head.completions == head.members and head.n == 3
    e.run_until_idle()
    assert m.prefills == [(0, [20])] and m.forks == [(0, [1, 2], 20, 0)]              # ONE prefill, one fork; pad = column - S
    assert [m.sampling_rows[r]["seed"] for r in (0, 1, 2)] == [41, 42, 43]
    assert all(m.sampling_rows[r]["counter"] == 0 for r in (0, 1, 2))                 # draw 0: from the prefill row
    assert head.family_done.is_set() and all(c.done.is_set() and c.error is None for c in head.completions)
    toks = [c.tokens for c in head.completions]
    assert len({tuple(t) for t in toks}) == 3                                          # three seeds, three texts
    assert all(len(t) == 30 or t[-1] == EOS for t in toks)
    # each member is the single request with its own seed
    for j, c in enumerate(head.completions):
        m1, e1 = _engine(1)
        solo = e1.submit(req(20, 1), 30, sampling={"temperature": 0.8, "seed": 41 + j})
        e1.run_until_idle()
        assert solo.tokens == c.tokens and solo.completions == [solo] and solo.family_done is solo.done
    # greedy family: n equal completions, the plain prefill call (no logits asked), no sampling records touched
    m, e = _engine(4)
    head = e.submit(n_args(req(20, 1), 3), 12)
    e.run_until_idle()
    assert m.forks == [(0, [1, 2], 20, 0)] and m.sampling_rows == {}
    assert head.completions[0].tokens == head.completions[1].tokens == head.completions[2].tokens and len(head.tokens) >= 1


def test_members_release_their_rows_independently_and_family_done_waits_for_the_last():
    from phi_3_vision_mlx_amd.engine import n_args
    m, e = _engine(3)
    head = e.submit(n_args(req(20, 1), 3), 200, sampling={"temperature": 0.8, "seed": 5})
    ends = {}
    for _ in range(400):
        if not (e.step() or e.waiting):
            break
        for j, c in enumerate(head.members):
            if c.done.is_set() and j not in ends:
                ends[j] = e.steps
                assert e.rows[c.row] is not c                                          # its row is free the moment it ends
        assert head.family_done.is_set() == (len(ends) == 3)
    assert len(ends) == 3 and len(set(ends.values())) > 1, ends                          # different seeds reach EOS at different steps
    assert head.family_done.is_set()
    # a single request takes a row a member left, while the others are still generating
    m, e = _engine(3)
    head = e.submit(n_args(req(20, 1), 3), 200, sampling={"temperature": 0.8, "seed": 5})
    late = e.submit(req(10, 9), 4)
    while not any(c.done.is_set() for c in head.members):
        e.step()
    assert not head.family_done.is_set() and not late.done.is_set()
    e.run_until_idle()
    assert late.error is None and late.row in {c.row for c in head.members} and head.family_done.is_set()


def test_admission_all_or_nothing_fifo_and_patience():
    from phi_3_vision_mlx_amd.engine import n_args
    m, e = _engine(4, patience=3)
    a = [e.submit(req(30, i), 40) for i in range(2)]                                   # two rows busy
    e.step()
    fam = e.submit(n_args(req(20, 7), 3), 6)                                            # needs 3 rows, 2 are free: waits whole
    single = e.submit(req(12, 8), 5)                                                    # newer, fits one row: may overtake for `patience` steps
    e.step()
    assert all(c.row is None for c in fam.members) and m.forks == [] and single.row is not None
    assert fam.blocked_at is not None
    later = []
    for _ in range(6):
        later.append(e.submit(req(9, 20 + len(later)), 2))
        e.step()
    # after `patience` steps nothing newer is admitted: the engine drains for the family
    assert any(h.row is None and not h.done.is_set() for h in later), [h.row for h in later]
    e.run_until_idle()
    assert fam.family_done.is_set() and all(c.error is None for c in fam.members) and len(m.forks) == 1
    assert len(set(m.forks[0][1]) | {m.forks[0][0]}) == 3
    assert all(h.done.is_set() and h.error is None for h in a + [single] + later)
    # the rows of a family need not be adjacent
    m, e = _engine(5)
    hold = [e.submit(req(30, i), 50) for i in range(5)]
    e.step()
    for i in (0, 2, 4):
        hold[i].cancel()
    fam = e.submit(n_args(req(20, 7), 3), 4)
    e.step(), e.step()
    assert sorted(c.row for c in fam.members) == [0, 2, 4] and m.forks[-1][:2] == (0, [2, 4])
    # n > slots fails at submit; n == slots is fine
    m, e = _engine(2)
    big = e.submit(n_args(req(20, 7), 3), 4)
    assert big.done.is_set() and big.family_done.is_set() and isinstance(big.error, ValueError) and "n > slots" in str(big.error)
    assert not e.waiting
    ok = e.submit(n_args(req(20, 7), 2), 4)
    e.run_until_idle()
    assert ok.family_done.is_set() and ok.error is None
    for bad, word in (({"n": 0}, "1..16"), ({"n": 2, "best_of": 1}, "n..16"), ({"n": 2, "extra": 1}, "n_args"), ("3", "n_args")):
        from phi_3_vision_mlx_amd.engine import N_ARGS
        h = e.submit(dict(req(20, 7), **{N_ARGS: bad}), 4)
        assert h.done.is_set() and isinstance(h.error, ValueError) and word in str(h.error), (bad, h.error)
    st = e.st
    st.mlx4 = True
    h = e.submit(n_args(req(20, 7), 2), 4)
    assert isinstance(h.error, ValueError) and "mlx4" in str(h.error)


def test_cancel_failed_prefill_and_failed_step_clean_up_the_whole_family():
    from phi_3_vision_mlx_amd.engine import n_args
    # a cancelled head cancels the family, waiting or running
    m, e = _engine(3)
    head = e.submit(n_args(req(20, 1), 3), 500, sampling={"temperature": 0.8, "seed": 3})
    e.step(), e.step()
    assert any(e.rows[c.row] is c for c in head.members)       # (the stub's rows reach EOS within 29 steps, some at once)
    head.cancel()
    e.step()
    assert e.rows == [None] * 3 and head.family_done.is_set() and all(c.done.is_set() for c in head.members)
    m, e = _engine(3)
    block = e.submit(next(r for r in (req(30, s) for s in range(2, 60)) if int(r["input_ids"].sum()) % 29 < 15), 50)   # (no EOS for 13 steps)
    e.step()
    head = e.submit(n_args(req(20, 1), 3), 5)
    e.step()
    head.cancel()
    e.step()
    assert head.family_done.is_set() and all(c.done.is_set() and c.row is None for c in head.members) and not e.waiting
    # a failed prefill (here: the fork) releases every row and fails every member; the engine lives on
    m, e = _engine(3)
    m.fail_fork = True
    head = e.submit(n_args(req(20, 1), 3), 5, sampling={"temperature": 0.8, "seed": 3})
    e.step()
    assert head.family_done.is_set() and all(isinstance(c.error, RuntimeError) and c.done.is_set() for c in head.members)
    assert e.rows == [None] * 3 and e.st.pad_len.tolist() == [4096] * 3 and e.failures == 0
    m.fail_fork = False
    bad = req(20, 1)
    bad["input_ids"][0, 3] = 666                                                        # the stub's prefill raises on it
    head = e.submit(n_args(bad, 2), 5)
    nxt = e.submit(n_args(req(20, 4), 3), 5)
    e.run_until_idle()
    assert isinstance(head.error, ValueError) and head.family_done.is_set() and all(c.error is head.error for c in head.members)
    assert nxt.family_done.is_set() and all(c.error is None and c.tokens for c in nxt.members)
    # a step that raises fails running and waiting families alike
    m, e = _engine(3)
    run, wait = e.submit(n_args(req(20, 1), 3), 50), e.submit(n_args(req(20, 2), 2), 50)
    e.step()
    m.fail_next_step = True
    e.safe_step()
    for h in (run, wait):
        assert h.family_done.is_set() and all(c.done.is_set() and isinstance(c.error, RuntimeError) for c in h.members)
    assert e.failures == 1 and e.dead is None


def test_best_of_ranks_members_by_their_records():
    from phi_3_vision_mlx_amd.engine import Request, make_family
    head = make_family(Request({"input_ids": np.zeros((1, 4), dtype=np.int64)}, 8, sampling=(1.0, 0, 1.0, 1)), 2, 4)
    scores = [[-1.0, -2.0], [-0.5, -0.25], [-0.5, -0.25], [-9.0]]
    for j, (c, s) in enumerate(zip(head.members, scores)):
        c.tokens = [10 + j] * len(s)
        c.logprob_records = [{"token": 10 + j, "logprob": x, "rank": 0, "top": []} for x in s]
    for c in reversed(head.members):
        assert not head.family_done.is_set()
        c.done.set()
        c.settle()
    assert head.family_done.is_set() and head.completions == [head.members[1], head.members[2]]      # tie: the lower index first
    # a member that failed ranks last, whatever its records say
    head = make_family(Request({"input_ids": np.zeros((1, 4), dtype=np.int64)}, 8), 1, 2)
    head.tokens, head.logprob_records, head.error = [1], [{"token": 1, "logprob": -0.1, "rank": 0, "top": []}], RuntimeError("x")
    other = head.members[1]
    other.tokens, other.logprob_records = [2], [{"token": 2, "logprob": -7.0, "rank": 3, "top": []}]
    for c in head.members:
        c.done.set()
        c.settle()
    assert head.completions == [other]
    # through the engine: five generated, the ranking function's three returned; the client asked for no records
    from phi_3_vision_mlx_amd.engine import n_args
    from phi_3_vision_mlx_amd.logprobs import rank_best_of
    m, e = _engine(6)
    head = e.submit(n_args(req(20, 1), 3, 5), 9, sampling={"temperature": 0.8, "seed": 2})
    assert head.completions is None and len(head.members) == 5
    e.run_until_idle()
    assert head.family_done.is_set() and all(len(c.logprob_records) == len(c.tokens) >= 1 for c in head.members)
    order = rank_best_of([c.tokens for c in head.members], [[r["logprob"] for r in c.logprob_records] for c in head.members], 3, EOS)
    assert head.completions == [head.members[j] for j in order] and head.asked_logprobs is None
    assert sorted(order) != order or len({tuple(c.tokens) for c in head.members}) > 1
    # a generated member whose step fails -- here the HEAD -- is ranked last and fails nobody that is returned
    m, e = _engine(6)
    head = e.submit(n_args(req(20, 1), 2, 4), 9, sampling={"temperature": 0.8, "seed": 2})
    e.step()
    live = [c for c in head.members if not c.done.is_set()]
    assert head in live and len(live) >= 3
    m.poison_row = head.row
    e.run_until_idle()
    assert head.family_done.is_set() and isinstance(head.error, RuntimeError) and head not in head.completions
    assert len(head.completions) == 2 and all(c.error is None and c.tokens for c in head.completions)


# ----------------------------------------------------------------------------- router and fleet: one engine per family
def test_router_and_fleet_keep_a_family_on_one_engine():
    from phi_3_vision_mlx_amd import fleet
    from phi_3_vision_mlx_amd.engine import ContinuousEngine, RegimeRouter, n_args
    ms, ml = ForkStub(), ForkStub()
    short, long_ = ContinuousEngine(ms, None, slots=4, window=4096), ContinuousEngine(ml, None, slots=4, window=8192)
    router = RegimeRouter([short, long_])
    a = router.submit(n_args(req(20, 1), 3), 10, sampling={"temperature": 0.8, "seed": 2})
    b = router.submit(n_args(req(20, 1), 2), 4200)                                     # prompt + max_tokens > 4096: the long engine
    while router.safe_step() or router.waiting:
        pass
    assert a.family_done.is_set() and b.family_done.is_set() and a.error is None and b.error is None
    assert ms.forks == [(0, [1, 2], 20, 0)] and ml.forks == [(0, [1], 20, 0)]           # each family whole, on ONE engine
    assert len(ms.prefills) == 1 and len(ml.prefills) == 1
    front = fleet.EngineFleet(short, (None, None), 1)                                   # world 1: rank 0's own engine
    ms.forks.clear()
    h = front.submit(n_args(req(20, 3), 3), 6)
    short.run_until_idle()
    assert h.family_done.is_set() and len(h.completions) == 3 and len(ms.forks) == 1 and front.sent == [1]
    bad = front.submit(n_args(req(20, 3), 0), 6)
    assert isinstance(bad.error, ValueError) and "1..16" in str(bad.error) and front.sent == [1]       # never left rank 0


def _fleet_worker(rank, world, port, out_dir):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "tests")]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from test_parallel_sampling_cpu import ForkStub
    from phi_3_vision_mlx_amd import fleet
    from phi_3_vision_mlx_amd.engine import ContinuousEngine, Request, n_args
    stub = ForkStub()
    eng = ContinuousEngine(stub, None, slots=4, window=4096)
    groups = fleet.make_groups()
    if rank:
        fleet.worker(eng, groups)
        open(os.path.join(out_dir, "forks"), "w").write(json.dumps(stub.forks))
        dist.destroy_process_group()
        return
    front = fleet.EngineFleet(eng, groups, world)
    stop = threading.Event()
    stepper = threading.Thread(target=front.serve_forever, args=(stop,), daemon=True)
    stepper.start()
    front.local = [Request(req(5, 0), 1) for _ in range(5)]                             # rank 0 looks loaded: the family goes to rank 1
    h = front.submit(n_args(req(20, 3), 2, 4), 6, sampling={"temperature": 0.8, "seed": 9})
    assert h.rank == 1 and h.family_done.wait(60) and h.error is None, h.error
    assert len(h.completions) == 2 and h.completions[0] is h and all(c.done.is_set() and c.tokens for c in h.completions)
    seeds = [c.sampling[3] for c in h.completions]
    assert len(set(seeds)) == 2 and set(seeds) <= {9, 10, 11, 12}                        # two of the four generated rows
    ref = ContinuousEngine(ForkStub(), None, slots=4, window=4096)
    r = ref.submit(n_args(req(20, 3), 2, 4), 6, sampling={"temperature": 0.8, "seed": 9})
    ref.run_until_idle()
    assert [c.tokens for c in r.completions] == [c.tokens for c in h.completions]
    assert [c.sampling[3] for c in r.completions] == seeds
    front.local = []
    front.close()
    stop.set()
    stepper.join(5)
    open(os.path.join(out_dir, "front"), "w").write(json.dumps(stub.forks))
    dist.destroy_process_group()


def test_fleet_two_ranks_sends_the_family_as_one_request(tmp_path):
    import torch.multiprocessing as mp
    from test_fleet_cpu import _free_port
    mp.spawn(_fleet_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    assert json.loads(open(tmp_path / "front").read()) == []                            # nothing ran on rank 0
    forks = json.loads(open(tmp_path / "forks").read())
    assert len(forks) == 1 and forks[0][:2] == [0, [1, 2, 3]]                            # one prefill row, forked into three, on rank 1


# ----------------------------------------------------------------------------- server
def _post(port, payload):
    r = urllib.request.Request(f"http://127.0.0.1:{port}/v1/completions", data=json.dumps(payload).encode(),
                               headers={"Content-Type": "application/json"})
    with urllib.request.urlopen(r, timeout=10) as resp:
        return resp.status, json.loads(resp.read())


def _expect_400(port, payload, word):
    with pytest.raises(urllib.error.HTTPError) as e:
        _post(port, payload)
    assert e.value.code == 400
    assert word in json.loads(e.value.read())["error"], json.loads(e.value.read() or b"{}")


def _serve_queue(**kw):
    from phi_3_vision_mlx_amd.server import serve
    calls = []

    def fake_generate(prompts, max_tokens, images=None, **kw_):
        calls.append((list(prompts), max_tokens, images, dict(kw_)))
        n = kw_.get("n")
        if n is None:
            out = [f"{p}|{max_tokens}" for p in prompts]
            return out[0] if len(out) == 1 else out
        if kw_.get("family_info") is not None and kw_.get("sampling"):
            kw_["family_info"].update(chosen=list(range(n)), seeds=[kw_["sampling"][0]["seed"] + 2 * j for j in range(n)])
        if kw_.get("logprob_info") is not None:
            kw_["logprob_info"].update(token_ids=[[j] for j in range(n)], token_logprobs=[[-0.5] for _ in range(n)],
                                       ranks=[[0] for _ in range(n)], top_logprobs=[[[]] for _ in range(n)])
        return [f"{prompts[0]}#{j}" for j in range(n)]
    httpd, engine = serve(fake_generate, port=0, host="127.0.0.1", **kw)
    threading.Thread(target=httpd.serve_forever, daemon=True).start()
    return httpd, engine, calls


def test_server_n_and_best_of_on_the_queue_path():
    httpd, engine, calls = _serve_queue(speculate=True, speculate_default=3, decode_fn=lambda i: f"<{i}>")
    port = httpd.server_address[1]
    try:
        # without "n": byte for byte today's response, and the stub sees exactly today's call
        assert _post(port, {"prompt": "hi", "max_tokens": 9, "speculate": 0})[1] == {"model": "phi-3-vision", "responses": ["hi|9"]}
        assert calls[-1] == (["hi"], 9, None, {})
        assert _post(port, {"prompt": "hi", "max_tokens": 9, "n": 1, "speculate": 0})[1] == {"model": "phi-3-vision", "responses": ["hi|9"]}
        assert calls[-1] == (["hi"], 9, None, {})                                         # n = 1: the same call
        assert _post(port, {"prompt": ["a", "b"], "max_tokens": 4, "n": 1})[1]["responses"] == ["a|4", "b|4"]
        # a family: n responses; the server-wide speculate default steps aside
        code, out = _post(port, {"prompt": "hi", "max_tokens": 9, "n": 3})
        assert code == 200 and out == {"model": "phi-3-vision", "responses": ["hi#0", "hi#1", "hi#2"]}
        assert calls[-1][3]["n"] == 3 and calls[-1][3]["best_of"] is None and "speculate" not in calls[-1][3]
        code, out = _post(port, {"prompt": "hi", "n": 2, "best_of": 5, "temperature": 0.7, "seed": 40, "logprobs": 1})
        assert out["responses"] == ["hi#0", "hi#1"] and out["seeds"] == [40, 42]          # the seeds of the RETURNED completions
        assert calls[-1][3]["n"] == 2 and calls[-1][3]["best_of"] == 5 and calls[-1][3]["sampling"][0]["seed"] == 40
        assert [o["token_ids"] for o in out["logprobs"]] == [[0], [1]] and out["logprobs"][1]["tokens"] == ["<1>"]
        assert _post(port, {"prompt": "hi", "best_of": 2})[1]["responses"] == ["hi#0"]    # n defaults to 1
        assert _post(port, {"prompt": "hi", "n": 1, "best_of": 1, "speculate": 0})[1]["responses"] == ["hi|512"]
        for bad, word in (({"n": 0}, "1..16"), ({"n": 17}, "1..16"), ({"n": "3"}, "integer"), ({"n": 2.0}, "integer"), ({"n": True}, "integer"),
                          ({"n": 3, "best_of": 2}, "n..16"), ({"best_of": 17}, "n..16"), ({"n": 2, "speculate": 4}, "speculative")):
            _expect_400(port, {"prompt": "hi", **bad}, word)
        _expect_400(port, {"prompt": ["a", "b"], "n": 2}, "one prompt")
        _expect_400(port, {"prompt": ["a"], "n": 2}, "one prompt")
    finally:
        httpd.shutdown()
        engine.close()
    httpd, engine, calls = _serve_queue(merge=True)
    try:
        _expect_400(httpd.server_address[1], {"prompt": "hi", "n": 2}, "--merge")
        assert _post(httpd.server_address[1], {"prompt": "hi", "n": 1})[0] == 200
    finally:
        httpd.shutdown()
        engine.close()


def test_server_n_on_the_continuous_backend():
    """The handler over server.ContinuousBackend over a real ContinuousEngine on the fake model: n texts, n seeds, and the
    plain request untouched."""
    from phi_3_vision_mlx_amd.engine import ContinuousEngine
    from phi_3_vision_mlx_amd.server import serve_continuous

    class Tok:
        def __call__(self, text):
            return type("E", (), {"input_ids": [5] + [3 + (ord(c) % 500) for c in text]})()

        def decode(self, ids, **kw):
            return " ".join(str(int(i)) for i in ids)

    class Proc:
        tokenizer = Tok()

        def __call__(self, text, images=None):
            return {"input_ids": np.asarray([self.tokenizer(text).input_ids], dtype=np.int64)}

    m = ForkStub()
    httpd, backend = serve_continuous(ContinuousEngine(m, Proc(), slots=4, window=4096), port=0)
    threading.Thread(target=httpd.serve_forever, daemon=True).start()
    port = httpd.server_address[1]
    try:
        plain = _post(port, {"prompt": "hello", "max_tokens": 5})[1]
        assert set(plain) == {"model", "responses"} and len(plain["responses"]) == 1 and m.forks == []
        out = _post(port, {"prompt": "hello", "max_tokens": 5, "n": 3, "temperature": 0.9, "seed": 7})[1]
        assert set(out) == {"model", "responses", "seeds"} and len(out["responses"]) == 3 and out["seeds"] == [7, 8, 9]
        assert len(m.forks) == 1 and len(set(out["responses"])) == 3
        for j, s in enumerate(out["seeds"]):                                              # each seed alone, n = 1: its text again
            again = _post(port, {"prompt": "hello", "max_tokens": 5, "n": 1, "temperature": 0.9, "seed": s})[1]
            assert again["responses"] == [out["responses"][j]] and again["seeds"] == [s]
        greedy = _post(port, {"prompt": "hello", "max_tokens": 5, "n": 2})[1]
        assert set(greedy) == {"model", "responses"} and greedy["responses"] == [plain["responses"][0]] * 2
        _expect_400(port, {"prompt": ["a", "b"], "n": 2}, "one prompt")
        with pytest.raises(urllib.error.HTTPError) as err:                               # the ENGINE's refusal (4 slots): the handle fails at submit
            _post(port, {"prompt": "hello", "n": 5})
        assert err.value.code == 500 and "n > slots" in json.loads(err.value.read())["error"]
    finally:
        httpd.shutdown()
        backend.close()
