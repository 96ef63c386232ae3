"""The per-row decode options around a prefill, stated once (sampling, penalties with logit_bias, guides, log-probabilities): what
they need on a state, in which order, before a row's first token is drawn; how that token and its record come out of the prefill
logits; how a row hands its tables over clean; how they are put back after a re-plan.  api._generate, api.greedy_loop and
ContinuousEngine pass rows, the requests' values (one per row), prompt and logits; all goes through the model's public methods.
Rows come as spans [(row0, n)]: a batch or a prefill group is ONE span, its tensors go to the model whole; a family is one
single-row span per member (its rows need not be adjacent; adjacent ones are not merged)."""
import numpy as np
import torch

from . import guide as guide_mod
from . import ops as model_ops
from . import penalties as penalties_mod
from . import sampling as sampling_mod

ID_EOS = 32007


class Asked:
    """What the requests of some rows ask, one value per row (None: not this row); a field is None when no row asks.  sampling:
    (temperature, top_k, top_p, seed); penalties: a penalties.rows row; guides: a guide.Dfa; wants: N, or -1.  lead_guide (a
    family): the guide goes to the first row alone, model.fork_rows hands region and start state to the others.  alone
    (api._generate): the rows are all of a state that this call alone steps -- nothing is vacated, and rows adjusted or masked
    but not sampled take the arg-max launch; in the engine they are drawn under greedy records (temperature 0: the same token)."""

    def __init__(self, sampling=None, penalties=None, guides=None, wants=None, lead_guide=False, alone=False):
        self.sampling, self.penalties, self.guides, self.wants = (
            None if v is None or all(x is None for x in v) else list(v) for v in (sampling, penalties, guides, wants))
        self.wants = self.wants and [-1 if w is None else w for w in self.wants]
        self.lead_guide, self.alone = lead_guide, alone
        self.drawn = self.sampling is not None or (not alone and (self.penalties is not None or self.guides is not None))

    @classmethod
    def of(cls, requests, lead_guide=False):
        return cls(*([getattr(r, f) for r in requests] for f in ("sampling", "penalties", "guide", "logprobs")), lead_guide=lead_guide)


def on_device(model, method=None, penalized=False, guided=False):
    """Does this model class carry the options on its states -- has it the step `method` a loop is to drive, or, where none is
    named, the setters of steps.NEEDS?  A class without keeps the eager launches of sampling and log-probabilities; penalties
    and guides have none."""
    ok = hasattr(model, method or "set_sampling")
    what = "penalties and logit_bias need" if penalized else "guided decoding needs" if guided else None
    if what and not ok:
        raise ValueError(f"{what} the device model's captured step (this model class has none)")
    return ok


def prompt_bits(inputs, rows=1):
    """(prompt ids int [n, S], per-row count of left-padding ids from the mask, or None): what a penalised row's `seen` bits
    start from.  ONE prompt for rows > 1 (a family): repeated, every row starts from the prompt's bits."""
    ids, mask = np.atleast_2d(np.asarray(inputs["input_ids"])), inputs.get("mask")
    pad = None if mask is None else (np.asarray(mask).reshape(ids.shape) == 0).sum(1).astype(np.int32)
    if rows > 1 and ids.shape[0] == 1:
        ids, pad = np.repeat(ids, rows, axis=0), (None if pad is None else np.repeat(pad, rows))
    return ids, pad


def _each(spans):                                              # [(row0, the slice of the per-row values)] of ONE span, or of single-row spans
    return [(row0, slice(i, i + n)) for i, (row0, n) in enumerate(spans)]


def install(model, st, spans, asked, inputs=None, processor=None):
    """Before the rows' first token is drawn (the engine: before their prefill): the tables the newcomers do not use are vacated
    where the state has them (a previous occupant may have used them), then guides (the vocabulary table once), penalties
    (records, the prompt bits of `inputs`, bias), then sampling records at draw counter 0 -- where the rows draw, and greedy
    ones where the state has records a sampled request may have left in these rows.  The wants follow the prefill."""
    each = _each(spans)
    for values, table, clear in ((asked.penalties, "penalty", "clear_penalties"), (asked.guides, "guide", "clear_guides")):
        if values is None and not asked.alone and getattr(st, table, None) is not None:
            for row0, n in spans:
                getattr(model, clear)(st, row0, n)
    if asked.guides is not None:
        model.set_guide_vocab(guide_mod.vocab_for(processor.tokenizer, model.cfg.vocab_size), ID_EOS)
        for row0, rows in each[:1 if asked.lead_guide else None]:
            model.set_guides(st, asked.guides[rows], row0)
    if asked.penalties is not None:
        prows = [p or penalties_mod.INACTIVE for p in asked.penalties]
        records, bias = penalties_mod.pack(prows), penalties_mod.bias_table(prows, model.cfg.vocab_size)
        ids, pad = prompt_bits(inputs, len(prows))
        kw_pad = {"pad": pad} if len(spans) == 1 else {}        # (a batch may be left-padded; a family's ONE prompt never is)
        for row0, rows in each:
            model.set_penalties(st, records[rows], ids[rows], row0, bias=None if bias is None else bias[rows], **kw_pad)
    if asked.drawn or (not asked.alone and getattr(st, "sample_rows", None) is not None):
        records = sampling_mod.pack([s or sampling_mod.GREEDY for s in asked.sampling or [None] * each[-1][1].stop], counter=0)
        for row0, rows in each:
            model.set_sampling(st, records[rows], row0)


def first_tokens(model, st, spans, asked, logits, toks=None):
    """The rows' first tokens from their prefill logits ([n, 1, V]; a family: its ONE row): adjusted where penalised, then
    masked where guided, then drawn under the rows' records -- or, where nothing draws, `toks`, the prefill's own arg-max
    (None: the arg-max launch, here); a negative token (NaN logits) raises.  Then the want entries and the tokens' records from
    the RAW logits.  A model class without the setters: the plain sample and log-probability launches.  -> (tokens int32 on
    the device, [n, 1] of one span and [n] of several; the same as a list; the records' words int32 [n, 20] or None)."""
    one, each, has = len(spans) == 1, _each(spans), logits is not None and on_device(model)
    if logits is not None and (asked.drawn or toks is None):
        drawn = []
        for row0, _ in each:
            first = logits
            if asked.penalties is not None:
                first = model.penalized_logits(st, first, row0)
            if asked.guides is not None:                        # behind the penalties: the mask works on the adjusted rows
                first = model.guided_logits(st, first, row0)
            last = first[:, -1, :] if first.dim() == 3 else first
            drawn.append(model.sample_logits(st, first, row0) if asked.drawn and has else
                         model_ops.sample(last, sampling_mod.pack(asked.sampling, counter=0).to(last.device))[:, None] if asked.drawn else
                         model_ops.argmax(last.contiguous())[:, None])
        toks = drawn[0] if one else torch.cat(drawn).reshape(-1)
    listed = toks.reshape(-1).tolist()
    if min(listed) < 0:
        raise RuntimeError(f"device prefill failed: NaN logits (token ids {listed})")
    if asked.wants is None or not has:                          # nobody asks; or the eager launch
        return toks, listed, asked.wants and model_ops.logprobs(logits[:, -1, :], toks.reshape(-1).to(torch.int32).contiguous(),
                                                                torch.tensor(asked.wants, dtype=torch.int32, device=logits.device))
    words = []
    for row0, rows in each:
        model.set_logprobs(st, asked.wants[rows], row0)
        words.append(model.logprobs_of(st, logits, toks if one else toks[rows], row0))
    return toks, listed, words[0] if one else torch.cat(words)


def release(model, st, row0, asked, if_made=False):
    """Rows row0 .. row0+n-1 stop carrying the options of the requests that held them: a row's next occupant costs the
    log-probability launch one early exit, and is neither penalised by this one's record nor masked by its guide.  Each table
    is touched only if one of the requests used it; if_made (a failed prefill, which may have stopped before a table was
    made): and only if the state has it."""
    for values, table, end in ((asked.wants, "logprob_want", lambda n: model.set_logprobs(st, [-1] * n, row0)),
                               (asked.penalties, "penalty", lambda n: model.clear_penalties(st, row0, n)),
                               (asked.guides, "guide", lambda n: model.clear_guides(st, row0, n))):
        if values is not None and not (if_made and getattr(st, table, None) is None):
            end(len(values))


def begin_loop(model, st, kind, token, sampling=None, wants=None, penalized=False, guided=False):
    """What the decode loop's steps read, written before the first of them: sampling records at draw counter 1 (the prefill token
    was draw 0), the wants, greedy records where the kind's tail is the sampled one and nobody samples.  -> (the model's step
    method of the kind, None, None); a model class without the setters: (None, records, wants) on the token's device, which
    ride with its eager loop."""
    records = None if sampling is None else sampling_mod.pack(sampling, counter=1)
    if not on_device(model, kind.method, penalized, guided):
        return (None, None if records is None else records.to(token.device),
                None if wants is None else torch.tensor(wants, dtype=torch.int32, device=token.device))
    if records is not None:
        model.set_sampling(st, records)
    if wants is not None:
        model.set_logprobs(st, wants)
    if kind.sampled and sampling is None:                       # the penalised / guided tail is the sampled one: greedy records
        model.set_sampling(st, sampling_mod.pack([sampling_mod.GREEDY] * token.shape[0], counter=1))
    return getattr(model, kind.method), None, None


def rebuild(model, st, n_done, fed, sampling=None, penalties=None, guides=None):
    """After a re-plan that rewound greedy_loop to step n_done: the tables may hold the dropped steps' draws, counts and walks.
    fed: per step 0 .. n_done-1 what the rows were FED (the prefill token, then the delivered ones; the next step notes its own)."""
    if sampling is not None:                                    # the draw index rewinds with the offset: step n_done draws n_done + 1
        model.set_sampling(st, sampling_mod.pack(sampling, counter=1 + n_done))
    if penalties is not None:                                   # rebuilt from the prompt and the tokens fed, rather than trusted
        model.rebuild_penalties(st, penalties["prompt_ids"], np.asarray(fed, dtype=np.int32).T if n_done else None, 0, penalties.get("pad"))
    if guides is not None:                                      # the states: walked again
        model.set_guides(st, guides["dfas"], 0, states=[
            guide_mod.replay_state(d, guides["table"], [f[b] for f in fed], guides["eos"]) for b, d in enumerate(guides["dfas"])])
