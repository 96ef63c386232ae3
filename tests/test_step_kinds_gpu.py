"""The eight step kinds on one state, in table order: the warm-up run that builds a kind's capture must leave everything it
moves -- the loop state, the sampling records' draw counters, the penalty state's `seen` table, the guide records -- as it found
it, so that after every step the state is what host-side counting says.  Teacher-forced: the test feeds every token itself."""
import numpy as np
import pytest
import torch

from phi_3_vision_mlx_amd import guide, penalties, sampling

pytestmark = pytest.mark.gpu
EOS = 32007
PROMPTS = ["<|user|>\nHi<|end|>\n<|assistant|>\n", "<|user|>\nWhy not?<|end|>\n<|assistant|>\n"]
# (method, sampled tail, penalised tail, guided tail, log-probability launch): steps.ALL's order, written out
ORDER = [("greedy_step", 0, 0, 0, 0), ("sample_step", 1, 0, 0, 0), ("logprob_step", 0, 0, 0, 1), ("sample_logprob_step", 1, 0, 0, 1),
         ("penal_step", 1, 1, 0, 0), ("penal_logprob_step", 1, 1, 0, 1), ("guide_step", 1, 1, 1, 0), ("guide_logprob_step", 1, 1, 1, 1)]
DIGITS = "3141592653589793"                                       # row 0 is fed these: "[0-9]+" accepts every prefix
OTHER = "the quick brown "                                        # row 1 (no guide, no penalty) is fed these


def _bits(t):
    return t.detach().contiguous().view(torch.int16).cpu().numpy().copy()


def test_every_kind_twice_leaves_the_state_as_counted():
    from phi_3_vision_mlx_amd import steps
    from phi_3_vision_mlx_amd.api import load_synthetic
    assert [k.method for k in steps.ALL] == [o[0] for o in ORDER]
    model, proc = load_synthetic(tiny=True, seed=0, std_scale=4.0, device="cuda:0")
    V = model.cfg.vocab_size
    table = guide.vocab_for(proc.tokenizer, V)
    one_byte = {table.bytes_of(i): i for i in reversed(range(256 + 64)) if len(table.bytes_of(i)) == 1}
    fed = [[one_byte[a.encode()], one_byte[b.encode()]] for a, b in zip(DIGITS, OTHER)]
    assert len(fed) == 2 * len(ORDER)
    dfa = guide.checked(guide.compile_regex("[0-9]+"), table, EOS)
    inputs = proc(PROMPTS, None)
    ids = np.asarray(inputs["input_ids"])
    pad = (np.asarray(inputs["mask"]).reshape(ids.shape) == 0).sum(1).astype(np.int32)
    assert pad.max() > 0                                          # (one row is left-padded: its pad ids must not be noted)

    _, cache = model(**inputs, max_tokens=20)
    _, twin = model(**inputs, max_tokens=20)                      # the same prompt, no option state, greedy_step alone
    st = cache[0].state
    prow = [(1.3, 0.2, 0.1, {5: -2.0, 48: 1.5}), penalties.INACTIVE]
    model.set_sampling(st, sampling.pack([(0.8, 40, 0.95, 7), (0.0, 0, 1.0, 0)], counter=1))
    model.set_penalties(st, penalties.pack(prow), ids, 0, bias=penalties.bias_table(prow, V), pad=pad)
    model.set_guide_vocab(table, EOS)
    model.set_guides(st, [dfa, None])
    model.set_logprobs(st, [2, -1])
    assert twin[0].state.sample_rows is None and twin[0].state.penalty is None and twin[0].state.guide is None

    n_sampled, fed_pen, fed_guide, hist, recs = 0, [], [], None, None
    for k, tok in enumerate(fed):
        method, sampled, penalized, guided, scored = ORDER[k // 2]       # each kind twice: its first use builds the capture
        token = torch.tensor(tok, dtype=torch.int32, device="cuda:0").view(2, 1)
        logits, nxt = getattr(model, method)(token, cache)
        torch.cuda.synchronize()
        want_logits, _ = model.greedy_step(token.clone(), twin)
        torch.cuda.synchronize()
        g = st.graphs["greedy"]
        n_sampled += sampled
        if penalized:
            fed_pen.append(tok)
        if guided:
            fed_guide.append(tok[0])
        what = (k, method)
        # the loop state: one step counted, one history column written, the cache one token longer
        assert int(g["d_step"].item()) == k + 1 and g["n_replays"] == k + 1 and st.offset == ids.shape[1] + k + 1, what
        assert int(g["d_past"].item()) == st.offset, what
        now = g["history"].clone()
        assert now[:, k].tolist() == nxt.reshape(-1).tolist(), what
        if hist is not None:
            now[:, k] = hist[:, k]
            assert torch.equal(now, hist), what                           # ... and no other column
        hist = g["history"].clone()
        # the records: one new column behind a log-probability launch (row 0 wants 2, row 1 nothing), none otherwise
        if "records" in g:
            new = g["records"].clone()
            if scored:
                assert int(new[0, k, 0]) == int(nxt[0, 0]) and int(new[0, k, 3]) == 2, what
                assert not new[1, k].any(), what
            if recs is not None:
                if scored:
                    new[:, k] = recs[:, k]
                assert torch.equal(new, recs), what
            recs = g["records"].clone()
        else:
            assert not scored, what
        # the draw counters: one per sampled tail, whatever the row's temperature
        assert [r["counter"] for r in sampling.unpack(st.sample_rows)] == [1 + n_sampled] * 2, what
        # the seen table: the prompt, then the tokens fed to penalised tails -- on the ACTIVE row (the rule's step 0: an inactive
        # row is copied through and counts nothing)
        seen = st.penalty["seen"].cpu().numpy().view(np.uint32)
        assert np.array_equal(seen[0], penalties.seen_table(ids[0, pad[0]:], [f[0] for f in fed_pen], V)), what
        assert np.array_equal(seen[1], penalties.seen_table(ids[1, pad[1]:], [], V)), what
        # the guide records: the walk of the tokens fed to guided tails
        assert st.guide["rows"].cpu().tolist() == [guide.record(dfa, guide.replay_state(dfa, table, fed_guide, EOS)), [0, 0, 0, 0]], what
        # the raw logits: those of the twin, bit for bit (a capture that disturbed the loop state or the cache would show here)
        assert np.array_equal(_bits(logits), _bits(want_logits)), what
    assert set(g) >= {"sample_graph", "logprob_graph", "sample_logprob_graph", "penal_graph", "penal_logprob_graph", "guide_graph",
                      "guide_logprob_graph"}
    assert guide.replay_state(dfa, table, fed_guide, EOS) not in (0, guide.DONE) and len(fed_guide) == 4 and len(fed_pen) == 8
