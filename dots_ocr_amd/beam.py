"""Beam search, stated on the host: the rule the engine's beam kernels implement, the float64 ranking of the hypotheses,
the exact early-termination test and the walk from a (step, beam) back to its tokens.  numpy only: no GPU, no torch.

These are vLLM's beam-search semantics with HF's length normalisation; they are not HF's BeamSearchScorer.

A group has width B.  cum[i] is an fp32 cumulative log-probability; at the start cum[0] = 0 and every other beam is dead (cum = -inf).
Per step every live beam i offers its 2B best (lp, id) pairs ordered by value descending, then id ascending.  A candidate is
(i, rank r, id, s = fp32(cum[i] + lp)); candidates of dead beams and candidates whose s is NaN or -inf do not exist.  A candidate whose
id is an EOS id is completed — recorded as (step, parent beam i, id, s) — and is no live candidate.  The B best others by (s descending,
i ascending, r ascending) are the new beams: beam j takes parent p_j, token t_j and cum[j] = s_j; with fewer than B candidates the
remaining beams are dead (parent and token read -1).  The group runs max_new steps, or until no beam is live."""
from typing import Callable, Iterable, List, Sequence, Tuple

import numpy as np

MAX_BEAMS = 8                                # DOTS_MAX_BEAMS, the engine's bound: 2B <= DOTS_MAX_TOP_LOGPROBS = 20 (the host model takes any B)

Completed = Tuple[int, int, int, np.float32]         # (step, parent beam, EOS id, cum)


def beam_search_host(top_fn: Callable, B: int, max_new: int, eos_ids: Iterable[int]):
    """top_fn(prefix) -> (ids, lps float32): the sorted top list of the next-token distribution after the generated tokens `prefix` (a
    tuple), of which the first 2B places count; an id of -1 is an empty place.  Returns (completed, trace): the completed records in (step, beam, rank)
    order and trace = {"parents": int32 [B, steps], "tokens": int32 [B, steps], "cum": float32 [steps, B]}, steps = the steps taken."""
    if B < 1:
        raise ValueError(f"a beam group has at least one beam, got {B}")
    eos = {int(t) for t in eos_ids}
    cum = np.full((B,), -np.inf, np.float32)
    cum[0] = 0.0
    prefixes: List[tuple] = [()] * B
    completed: List[Completed] = []
    parents, tokens, cums = [], [], []
    for step in range(int(max_new)):
        cands = []
        for i in range(B):
            if not cum[i] > -np.inf:
                continue
            ids, lps = top_fn(prefixes[i])
            for r in range(min(2 * B, len(ids))):
                tok = int(ids[r])
                if tok < 0:
                    continue
                s = np.float32(cum[i] + np.float32(lps[r]))
                if not s > -np.inf:                  # NaN or -inf
                    continue
                if tok in eos:
                    completed.append((step, i, tok, s))
                else:
                    cands.append((s, i, r, tok))
        cands.sort(key=lambda c: (-float(c[0]), c[1], c[2]))
        best = cands[:B]
        par = np.full((B,), -1, np.int32)
        tok = np.full((B,), -1, np.int32)
        new_cum = np.full((B,), -np.inf, np.float32)
        new_prefixes: List[tuple] = [()] * B
        for j, (s, i, _, t) in enumerate(best):
            par[j], tok[j], new_cum[j] = i, t, s
            new_prefixes[j] = prefixes[i] + (t,)
        parents.append(par)
        tokens.append(tok)
        cums.append(new_cum)
        cum, prefixes = new_cum, new_prefixes
        if not best:
            break
    steps = len(parents)
    trace = {"parents": np.stack(parents, 1) if steps else np.zeros((B, 0), np.int32),
             "tokens": np.stack(tokens, 1) if steps else np.zeros((B, 0), np.int32),
             "cum": np.stack(cums, 0) if steps else np.zeros((0, B), np.float32)}
    return completed, trace


def backtrace(parents, tokens, step: int, beam: int) -> List[int]:
    """The tokens of the hypothesis that is beam `beam` after step `step`: tokens[., 0 .. step] along its parents.  step = -1: none."""
    out = []
    b = int(beam)
    for t in range(int(step), -1, -1):
        if b < 0:
            raise ValueError(f"beam {beam} of step {step} descends from a dead beam at step {t}")
        out.append(int(tokens[b][t]))
        b = int(parents[b][t])
    return out[::-1]


def _score(cum, length: int, length_penalty: float) -> float:
    return float(cum) / float(max(1, int(length))) ** float(length_penalty)


def rank_hypotheses(completed: Sequence[Completed], parents, tokens, cum, steps: int, length_penalty: float = 1.0, num_return: int = 1) -> List[dict]:
    """The hypotheses of a group that ran `steps` steps, best first: the completed records and — with their cum — the beams still live.
    score = cum / max(1, len) ** length_penalty in float64, len = generated tokens without a final EOS; ranked by (score descending,
    completion step ascending, beam ascending), a live beam's completion step being `steps`.  Each is {"tokens" (the EOS included),
    "cum", "score", "step", "beam", "finish_reason": "stop" | "length"}; the best num_return are returned."""
    hyps = []
    for step, beam, tok, s in completed:
        if step < steps:
            hyps.append((-_score(s, step, length_penalty), int(step), int(beam), "stop", int(tok), s))
    for j in range(len(cum)):
        if steps > 0 and cum[j] > -np.inf:
            hyps.append((-_score(cum[j], steps, length_penalty), int(steps), j, "length", -1, cum[j]))
    hyps.sort(key=lambda h: h[:3])
    out = []
    for neg, step, beam, reason, tok, s in hyps[:max(0, int(num_return))]:
        if reason == "stop":
            toks = backtrace(parents, tokens, step - 1, beam) + [tok]
        else:
            toks = backtrace(parents, tokens, steps - 1, beam)
        out.append({"tokens": toks, "cum": float(s), "score": -neg, "step": step, "beam": beam, "finish_reason": reason})
    return out


def may_stop(completed: Sequence[Completed], live_cum, max_new: int, length_penalty: float, num_return: int) -> bool:
    """May the group end now without changing what rank_hypotheses returns at the cap?  Exact for length_penalty >= 0: a log-probability
    is <= 0, so no hypothesis that descends from a live beam can score above best_live_cum / max_new ** length_penalty; true when
    num_return completed hypotheses already score strictly above that, or no beam is live.  A negative penalty rewards length: false."""
    if length_penalty < 0:
        return False
    live = [float(c) for c in live_cum if c > -np.inf]
    if not live:
        return True
    bound = max(live) / float(max(1, int(max_new))) ** float(length_penalty)
    above = sum(1 for step, _, _, s in completed if _score(s, step, length_penalty) > bound)
    return above >= int(num_return)
