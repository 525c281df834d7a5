"""What an admission leaves behind does not depend on what the slot held before.  Every way a sequence enters a decode slot — one-shot
prefill, chunked fill, fork, beam group, extend — runs once on a fresh engine and once on an engine whose slot 3 has a history (a
sampled, penalised, logprob-returning sequence that ran to its cap, was read and released), and everything the API shows of the
admitted row must be equal bit for bit, right after the admission and after four more decode steps.  Prompt lengths: 70 (one full KV
page and a tail: fork and beam share a page and copy one) and 64 (the prompt ends on the page boundary: no tail copy).

Two reads of a beam group's child row are left out, because there the slot's history does show: creating a group writes no logits into
the child's row (its first selection reads the source's), so slot_logits of the child shows the row's earlier content until the first
decode step; and a group row returns no logprobs, yet row_logprobs of one reads the positions its previous occupant wrote.  The child's
logits are compared after the decode steps, the source's right after the admission."""
import numpy as np
import pytest

from dots_ocr_amd.config import DotsConfig
from dots_ocr_amd.engine import SamplingParams
from dots_ocr_amd.weights import random_state_dict

pytestmark = pytest.mark.gpu

SLOT, SRC = 3, 0                     # the admitted slot; the source of a fork or a group
MAX_NEW, TOP_N, L_HIST = 6, 2, 130
FED = [5, 9, 2, 7, 11]               # the tokens an extend feeds
_SD = {}


def _engine():
    from dots_ocr_amd.engine import Engine
    cfg = DotsConfig.tiny()
    if not _SD:
        _SD["sd"] = random_state_dict(cfg, seed=11)
    e = Engine(cfg, max_batch=8, max_seq_len=256, max_patches=4096, max_prefill_tokens=256)
    e.load_state_dict(_SD["sd"])
    e.set_eos([])
    return cfg, e


def _prompt(cfg, L):
    return np.random.default_rng(5200 + L).integers(0, cfg.vocab_size - 8, L).astype(np.int32)


def _history(cfg, e):
    """slot 3 held a sequence with penalty state, logprob positions and a finished flag, and was released"""
    e.set_row_sampling(SLOT, SamplingParams(temperature=0.8, seed=31, repetition_penalty=1.3))
    e.set_row_logprobs(SLOT, TOP_N)
    e.slots_prefill([SLOT], _prompt(cfg, L_HIST), [L_HIST], [MAX_NEW])
    e.slots_decode(MAX_NEW - 1)
    fin, lens = e.slots_poll()
    assert fin[SLOT] == 1 and lens[SLOT] == MAX_NEW, (fin, lens)
    assert len(e.slot_read(SLOT, MAX_NEW)) == MAX_NEW
    tok_lp = e.row_logprobs(SLOT, MAX_NEW)[0]
    assert len(tok_lp) == MAX_NEW and np.isfinite(tok_lp).all()
    e.slot_release(SLOT)


def _one_shot(cfg, e, L):
    e.set_row_logprobs(SLOT, TOP_N)
    e.slots_prefill([SLOT], _prompt(cfg, L), [L], [MAX_NEW])
    return L


def _chunked(cfg, e, L):
    e.set_row_logprobs(SLOT, TOP_N)
    e.slots_prefill_chunked([SLOT], _prompt(cfg, L), [L], [MAX_NEW], 64)
    return L


def _fork(cfg, e, L):
    e.set_row_logprobs(SLOT, TOP_N)
    e.slots_prefill([SRC], _prompt(cfg, L), [L], [MAX_NEW])
    e.slots_fork(SRC, [SLOT])
    return L


def _beam(cfg, e, L):
    e.slots_prefill([SRC], _prompt(cfg, L), [L], [MAX_NEW])
    e.slots_beam(SRC, [SLOT])
    return L


def _extend(cfg, e, L):
    e.set_row_logprobs(SLOT, TOP_N)
    e.slots_prefill([SLOT], _prompt(cfg, L), [L], [MAX_NEW])
    e.slots_decode(2)
    e.slots_extend([SLOT], [FED], keep_pending=False, max_new_tokens=MAX_NEW)
    return L + 2 + len(FED)


ADMISSIONS = {"one_shot": _one_shot, "chunked": _chunked, "fork": _fork, "beam": _beam, "extend": _extend}


def _snapshot(e, group, stepped):
    fin, lens = e.slots_poll()
    snap = {"finished": fin, "out_lens": lens, "capacity": np.asarray(e.slot_capacity(SLOT), np.int64), "tokens": e.slot_read(SLOT, MAX_NEW)}
    if not group:
        snap["tok_lp"], snap["top_ids"], snap["top_lp"] = e.row_logprobs(SLOT, MAX_NEW)
    if stepped or not group:
        snap["logits"] = e.slot_logits(SLOT)
    if group:
        snap["src_logits"] = e.slot_logits(SRC)
        tr = e.beam_read(SLOT)
        snap.update({"beam_" + k: np.asarray(tr[k]) for k in ("B", "steps", "cum", "tokens", "parents")})
        snap["beam_completed"] = np.asarray([(s, p, i, np.float32(c).view(np.uint32)) for s, p, i, c in tr["completed"]], np.int64).reshape(-1, 4)
    return snap


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _run(kind, L, history):
    cfg, e = _engine()
    try:
        if history:
            _history(cfg, e)
        prompt = ADMISSIONS[kind](cfg, e, L)
        first = _snapshot(e, kind == "beam", False)
        e.slots_decode(4)
        return prompt, first, _snapshot(e, kind == "beam", True)
    finally:
        e.close()


@pytest.mark.parametrize("L", [70, 64])
@pytest.mark.parametrize("kind", list(ADMISSIONS))
def test_admission_ignores_the_slots_history(kind, L):
    _, fresh_first, fresh_later = _run(kind, L, history=False)
    prompt, first, later = _run(kind, L, history=True)
    differing = []
    for when, a, b in (("after admission", fresh_first, first), ("after 4 steps", fresh_later, later)):
        assert a.keys() == b.keys()
        for k in a:
            same = np.shape(a[k]) == np.shape(b[k]) and np.array_equal(_bits(a[k]), _bits(b[k]))
            print(f"{kind} L={L} {when}: {k} {'equal' if same else 'DIFFERS'}")
            if not same:
                differing.append((when, k, a[k], b[k]))
    assert not differing, differing
    # ---- the absolute facts, on the engine with the history
    assert first["finished"][SLOT] == 0 and first["out_lens"][SLOT] == 1, (first["finished"], first["out_lens"])
    assert later["finished"][SLOT] == 0 and later["out_lens"][SLOT] == 5, (later["finished"], later["out_lens"])
    assert first["capacity"][1] == prompt + MAX_NEW
    if kind == "beam":
        # the group's first selection: the source's two most likely tokens, in order (the source's row holds the prompt's last-position logits)
        best = np.argsort(-first["src_logits"].astype(np.float64), kind="stable")[:2]
        assert first["beam_steps"] == 1 and first["beam_tokens"][:, 0].tolist() == best.tolist()
        assert first["tokens"].tolist() == [int(best[1])]
        return
    assert first["tokens"].tolist() == [int(np.argmax(first["logits"]))]
    # logprobs: exactly the generated positions exist, and every entry beyond the row's top_n is unset
    for snap, n in ((first, 1), (later, 5)):
        assert len(snap["tok_lp"]) == n and snap["top_ids"].shape == snap["top_lp"].shape == (n, 20)
        assert (snap["top_ids"][:, TOP_N:] == -1).all() and np.isnan(snap["top_lp"][:, TOP_N:]).all()
        assert np.isfinite(snap["tok_lp"]).all() and (snap["top_ids"][:, :TOP_N] >= 0).all() and np.isfinite(snap["top_lp"][:, :TOP_N]).all()
