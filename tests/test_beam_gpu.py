"""Beam search on a tiny synthetic model: every eager step's record against beam.reference_step on the step's own logits and
the caches against torch.index_select of their clones; the captured replay against the eager run, bit for bit; the public
call against beam.Search on those records; num_beams=1 against the plain call; a family-registered state against a plain
one; the refusals that need a model."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EOS = 32007
W, N_TOK = 4, 6
PROMPT = "<|user|>\nName three colours of the rainbow.<|end|>\n<|assistant|>\n"


def bits_of(t):
    return t.detach().contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


@pytest.fixture(scope="module")
def tiny():
    from phi_3_vision_mlx_amd.api import load_synthetic
    return load_synthetic(blind_model=True, tiny=True, seed=0, std_scale=4.0, device=DEV)


def _start(model, proc, W=W, n_tok=N_TOK, share=False):
    logits, cache = model(**proc(PROMPT), max_tokens=n_tok)
    row = logits[:, -1, :].contiguous()
    g = model.beam_start(cache, row, W, EOS, share=share)
    return row, g


@pytest.fixture(scope="module")
def eager_run(tiny):
    """N_TOK records from eager steps, every step checked on the way; the final caches."""
    from phi_3_vision_mlx_amd import beam, ops
    model, proc = tiny
    row, g = _start(model, proc)
    st = g["cache"][0].state
    torch.cuda.synchronize()
    S0, c0a = st.offset, g["c0a"]
    assert g["rec"][0].numpy().tolist() == beam.reference_step(bits_of(row), np.zeros(1, np.float32), W, EOS).tolist()
    assert int(g["d_past"][0]) == S0 and int(g["d_step"][0]) == 1 and int(g["ticket"][0]) == 0
    forward, select, reorder = g["parts"]
    for t in range(1, N_TOK):
        cum_in = g["cum"].cpu().numpy().copy()
        with ops.owned_gemm_workspace(g["gemm_ws"], frozen=True):
            forward()
        select()
        torch.cuda.synchronize()
        ref = beam.reference_step(bits_of(g["logits"]), cum_in, W, EOS)
        assert g["rec"][t].numpy().tolist() == ref.tolist(), t
        assert g["tok"].tolist() == ref[2:2 + W].tolist() and g["parent"].tolist() == ref[10:10 + W].tolist()
        assert int(g["d_past"][0]) == S0 + t and int(g["d_step"][0]) == t + 1
        k0, v0 = st.k.clone(), st.v.clone()
        reorder()
        torch.cuda.synchronize()
        parent = g["parent"].long()
        end = min((S0 + t + 7) // 8 * 8, st.Tp)
        assert c0a <= S0 < end
        want_k, want_v = k0.clone(), v0.clone()
        want_k[:, :, :, c0a:end] = k0.index_select(1, parent)[:, :, :, c0a:end]
        want_v[..., c0a:end] = v0.index_select(1, parent)[..., c0a:end]
        assert torch.equal(st.k.view(torch.int16), want_k.view(torch.int16)), t
        assert torch.equal(st.v.view(torch.int16), want_v.view(torch.int16)), t
        g["n_replays"] += 1
    recs = model.beam_sync(g["cache"])
    assert st.offset == S0 + N_TOK - 1 and recs.shape == (N_TOK, beam.REC_INTS)
    return recs, st.k[..., :st.offset, :].clone(), st.v[..., :st.offset].clone()


def test_eager_steps_obey_the_rule_and_reorder_the_rows(eager_run):
    from phi_3_vision_mlx_amd import beam
    recs = eager_run[0]
    assert (recs[:, 0] == 0).all()
    parents = [beam.unpack(r, W)["parent"] for r in recs[1:]]
    assert any(p != list(range(W)) for p in parents)                     # rows did move


def test_captured_replay_is_bit_identical_to_the_eager_steps(tiny, eager_run):
    model, proc = tiny
    _, g = _start(model, proc)
    for _ in range(N_TOK - 1):
        model.beam_step(g["cache"])
    recs = model.beam_sync(g["cache"])
    st = g["cache"][0].state
    assert np.array_equal(recs, eager_run[0])
    assert torch.equal(st.k[..., :st.offset, :].view(torch.int16), eager_run[1].view(torch.int16))
    assert torch.equal(st.v[..., :st.offset].view(torch.int16), eager_run[2].view(torch.int16))
    with pytest.raises(ValueError, match="overflow"):                    # the budget: no step beyond prompt + max_tokens
        model.beam_step(g["cache"])
    # overrun records are dropped and the offset rewound past them
    model.beam_sync(g["cache"], 3)
    assert st.offset == g["S0"] + 2


def test_family_registered_state_gives_the_same_records(tiny, eager_run, monkeypatch):
    from phi_3_vision_mlx_amd import model as model_mod
    model, proc = tiny
    monkeypatch.setattr(model_mod, "family_pays", lambda n, keys: True)  # (a short prompt lies below the measured break-even)
    runs = []
    for clear in (False, True):
        _, g = _start(model, proc, share=True)
        st = g["cache"][0].state
        assert g["bufs"]["plan"].family and st.families
        if clear:                                                        # the same launch and split plan, every row on its own
            model.set_families(st, [])
            assert not st.families
        for _ in range(N_TOK - 1):
            model.beam_step(g["cache"])
        runs.append(model.beam_sync(g["cache"]))
    assert np.array_equal(runs[0], runs[1])
    assert np.array_equal(runs[0], eager_run[0])                         # the plain state: no family, the same launch and plan


@pytest.mark.parametrize("length_penalty", [1.0, 0.0])
def test_generate_returns_what_search_makes_of_the_records(tiny, eager_run, length_penalty):
    from phi_3_vision_mlx_amd import api, beam
    model, proc = tiny
    search = beam.Search(W, N_TOK, EOS, length_penalty)
    for r in eager_run[0]:
        if search.add(r):
            break
    want = search.result()
    info = {}
    txt = api.generate(PROMPT, preload=(model, proc), max_tokens=N_TOK, num_beams=W, length_penalty=length_penalty, beam_info=info,
                       verbose=False, stream=False, apply_chat_template=False)
    assert info["hypotheses"] == want and info["steps"] == len(search.steps)
    assert txt == proc.tokenizer.decode(want[0]["token_ids"])
    assert set(info["hypotheses"][0]) == {"token_ids", "score", "sum_logprob", "finished"} and len(want) == W
    assert [h["score"] for h in want] == sorted((h["score"] for h in want), reverse=True)


def test_num_beams_one_is_the_plain_call():
    from phi_3_vision_mlx_amd import api
    model, proc = api.load_synthetic(blind_model=True, tiny=True, seed=0, std_scale=4.0, device=DEV)
    kw = dict(max_tokens=N_TOK, verbose=False, stream=False, mute=True)
    plain = api._generate(model, proc, PROMPT, **kw)
    one = api._generate(model, proc, PROMPT, num_beams=1, length_penalty=2.0, **kw)
    assert one == plain
    states = list(model._states)
    assert states and all(not any("beam" in str(k) for k in s.graphs) and s.family is None for s in states)
    info = {}
    api._generate(model, proc, PROMPT, num_beams=2, beam_info=info, **kw)
    assert any(("beam", 2) in s.graphs for s in model._states) and info["steps"] >= 1


def test_refusals_that_need_a_model(tiny):
    from phi_3_vision_mlx_amd import api
    model, proc = tiny
    kw = dict(max_tokens=4, verbose=False, stream=False, mute=True)
    for cfg_kw, word in ((dict(use_quantized_cache=True), "int8"), (dict(use_quantized_cache=True, cache_format="mlx4"), "mlx4")):
        m2, p2 = api.load_synthetic(blind_model=True, tiny=True, seed=0, device=DEV, **cfg_kw)
        with pytest.raises(ValueError, match=word):
            api._generate(m2, p2, PROMPT, num_beams=2, **kw)
    with pytest.raises(ValueError, match=r"2\.\.8"):
        api._generate(model, proc, PROMPT, num_beams=9, **kw)
    with pytest.raises(ValueError, match="max_tokens"):
        api._generate(model, proc, PROMPT, num_beams=2, **dict(kw, max_tokens=0))
    logits, cache = model(**proc(PROMPT), max_tokens=4)
    with pytest.raises(ValueError, match=r"2\.\.8"):
        model.beam_start(cache, logits[:, -1, :], 1, EOS)
    logits2, cache2 = model(**proc([PROMPT, PROMPT]), max_tokens=4)
    with pytest.raises(ValueError, match="B = 1"):
        model.beam_start(cache2, logits2[0, -1, :], 2, EOS)
    with pytest.raises(RuntimeError, match="beam_start"):
        model.beam_step(cache)
