"""The kinds of the captured decode step, stated once (model.py builds and replays them, engine.py and api.py pick one).

A step has a TAIL -- greedy (arg-max), sampled, penalised or guided; each later tail implies the earlier ones (the penalised
tail is the sampled one on adjusted logits, the guided tail the penalised one behind the mask) -- and is optionally followed by
the log-probability launch.  That leaves eight kinds.  A new per-row option is added HERE: a flag, its rows in the table, what
it needs on the state (NEEDS); model.py then says what its warm-up run moves and what `_decode_step` launches for it.
No torch in this module: it is names and booleans.
"""
import dataclasses

FLAGS = ("sampled", "penalized", "guided", "logprobs")

# flag -> what a step with it reads on the state (a CacheState attribute, None until made) and the model's setter that makes it
NEEDS = (("sampled", "sample_rows", "set_sampling"), ("penalized", "penalty", "set_penalties"), ("guided", "guide", "set_guides"),
         ("logprobs", "logprob_want", "set_logprobs"))

# (sampled, penalized, guided, logprobs) -> the model's public method of the kind, and the key of its hipGraph in the state's
# greedy capture (`st.graphs["greedy"]`)
_TABLE = {
    (False, False, False, False): ("greedy_step", "graph"),
    (True, False, False, False): ("sample_step", "sample_graph"),
    (False, False, False, True): ("logprob_step", "logprob_graph"),
    (True, False, False, True): ("sample_logprob_step", "sample_logprob_graph"),
    (True, True, False, False): ("penal_step", "penal_graph"),
    (True, True, False, True): ("penal_logprob_step", "penal_logprob_graph"),
    (True, True, True, False): ("guide_step", "guide_graph"),
    (True, True, True, True): ("guide_logprob_step", "guide_logprob_graph"),
}


@dataclasses.dataclass(frozen=True)
class StepKind:
    """One kind of step, normalised on construction: guided implies penalized, penalized implies sampled.  `method` and `capture`
    are its row of the table."""
    sampled: bool = False
    penalized: bool = False
    guided: bool = False
    logprobs: bool = False
    method: str = dataclasses.field(init=False, compare=False, repr=False)
    capture: str = dataclasses.field(init=False, compare=False, repr=False)

    def __post_init__(self):
        guided = bool(self.guided)
        penalized = guided or bool(self.penalized)
        flags = (penalized or bool(self.sampled), penalized, guided, bool(self.logprobs))
        for name, v in zip(FLAGS + ("method", "capture"), flags + _TABLE[flags]):
            object.__setattr__(self, name, v)

    def missing(self, st):
        """The setters that have not been called on a state this kind is to run on."""
        return [setter for flag, attr, setter in NEEDS if getattr(self, flag) and getattr(st, attr) is None]

    def check(self, st):
        """RuntimeError -- before anything is launched -- when the state lacks something the step reads."""
        lack = self.missing(st)
        if lack:
            raise RuntimeError(f"{self.method}: nothing on this state for the step to read -- call model." + ", model.".join(lack) + " first")


ALL = tuple(StepKind(*flags) for flags in _TABLE)
GREEDY = ALL[0]

_TAILS = {0: "each row's token is the arg-max of its logits (reference phi_3_vision_mlx.py:391-392)",
          1: "each row's token is drawn under its sampling record (a T = 0 row: the arg-max)",
          2: "p3v_penalize counts the fed token and adjusts the rows, the sampled tail draws from the adjusted rows",
          3: "p3v_penalize, then p3v_guide_mask walks the fed token and bans what the new state does not allow, then the sampled "
             "tail on the adjusted rows"}


def kind_for(sampled=False, penalized=False, guided=False, scored=False):
    """The kind to replay for what the active rows -- or a loop's arguments -- ask: any row sampled / penalised / guided / scored."""
    return StepKind(sampled, penalized, guided, scored)


def with_flag(flag):
    """The kinds that have a flag set (by the normalisation, `penalized` names the guided kinds too)."""
    return [k for k in ALL if getattr(k, flag)]


def _method(kind):
    def step(self, token, cache):
        kind.check(cache[0].state)
        return self._replay(token, cache, kind)
    step.__name__ = kind.method
    step.__doc__ = (f"One decode step of the kind {kind} through its captured graph (built on first use over the greedy capture's "
                    f"loop state; kinds may alternate on one state): {_TAILS[kind.sampled + kind.penalized + kind.guided]}"
                    + (", followed by the log-probability launch on the RAW logits" if kind.logprobs else "")
                    + ".  Needs " + (", ".join(s for f, _, s in NEEDS if getattr(kind, f)) or "nothing")
                    + " on the state (steps.NEEDS).  Returns (raw logits [B,1,V], next_token [B,1]): views of persistent buffers, "
                    "valid until the next call.")
    return step


def methods(wrap=lambda fn: fn):
    """Class decorator: give a class with `_replay(token, cache, kind)` the eight public step methods of the table -- each checks
    what its kind needs on `cache[0].state`, then replays.  wrap: applied to every method (the model's device guard)."""
    def install(cls):
        for kind in ALL:
            fn = _method(kind)
            fn.__qualname__ = f"{cls.__qualname__}.{kind.method}"
            setattr(cls, kind.method, wrap(fn))
        return cls
    return install
