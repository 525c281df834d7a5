"""Beam search through the public surfaces on the GPU: modeling.generate(num_beams=) and a beam request in the
ContinuousBatcher return the ranked hypotheses that the host model derives from the engine's own unbeamed logprobs (the oracle of
tests/test_beam_gpu.py), and a call without num_beams is what it was."""
import numpy as np
import pytest
import torch

from dots_ocr_amd.beam import rank_hypotheses
from dots_ocr_amd.config import DotsConfig
from dots_ocr_amd.scheduler import ContinuousBatcher, Request
from dots_ocr_amd.weights import random_state_dict
from test_beam_gpu import _prompt, forced_table, oracle, run_group

pytestmark = pytest.mark.gpu

L, B, N_NEW, N_RET = 63, 3, 12, 2


def _model():
    from dots_ocr_amd.modeling import DotsOcrHipForCausalLM
    cfg = DotsConfig.tiny(layers=3, v_layers=3, vocab=1024)
    return cfg, DotsOcrHipForCausalLM(cfg, random_state_dict(cfg, seed=11), device=0, max_batch=8, max_seq_len=640, max_patches=4096)


@pytest.fixture(scope="module")
def case():
    """the model, a prompt, two EOS ids out of the root's top list (rank 1 and rank B + 1: hypotheses complete at once and later) and the
    hypotheses the oracle ranks for them, per length penalty"""
    cfg, model = _model()
    e = model.engine
    ids = _prompt(cfg, L, seed=5)
    root = forced_table(e, ids, {()}, N_NEW)[()]
    eos = [int(root[0][1]), int(root[0][B + 1])]
    tr = run_group(e, ids, [0, 1, 2], N_NEW, eos=eos)
    completed, host = oracle(e, ids, tr, N_NEW, eos=eos)
    assert np.array_equal(tr["tokens"], host["tokens"]) and np.array_equal(tr["parents"], host["parents"])

    def ranked(penalty):
        return rank_hypotheses(completed, host["parents"], host["tokens"], host["cum"][-1], host["tokens"].shape[1], penalty, N_RET)
    yield cfg, model, ids, eos, ranked
    e.close()


@pytest.mark.parametrize("penalty", [1.0, -0.5])             # ended early where that is exact / run to the cap
def test_generate_returns_the_ranked_hypotheses(case, penalty):
    cfg, model, ids, eos, ranked = case
    out = model.generate(input_ids=torch.from_numpy(ids.astype(np.int64))[None], max_new_tokens=N_NEW, eos_token_id=eos, num_beams=B,
                         num_return_sequences=N_RET, length_penalty=penalty)
    want = ranked(penalty)
    assert out.shape[0] == N_RET and out[:, :L].tolist() == [ids.tolist()] * N_RET
    for row, h in zip(out[:, L:].tolist(), want):
        assert row[:len(h["tokens"])] == h["tokens"] and all(t == cfg.pad_token_id for t in row[len(h["tokens"]):])
    assert {h["finish_reason"] for h in ranked(1.0)} | {h["finish_reason"] for h in ranked(-0.5)} == {"stop", "length"}


def test_generate_refuses_what_a_beam_row_cannot_honour(case):
    cfg, model, ids, eos, _ = case
    x = torch.from_numpy(ids.astype(np.int64))[None]
    for kw in (dict(early_stopping=True), dict(do_sample=True, temperature=0.7), dict(top_k=4), dict(repetition_penalty=1.2), dict(logit_bias={3: 1.0}),
               dict(min_tokens=2), dict(no_repeat_ngram_size=2), dict(stop_strings=["ab"]), dict(speculative_ngram=2), dict(continuous=False),
               dict(num_return_sequences=4), dict(num_beams=9)):
        with pytest.raises(ValueError):
            model.generate(input_ids=x, max_new_tokens=4, **{"num_beams": B, **kw})


def test_a_beam_request_beside_ordinary_requests(case):
    cfg, model, ids, eos, ranked = case
    e = model.engine
    others = [_prompt(cfg, 40, seed=6), _prompt(cfg, 90, seed=7)]
    e.set_sampling(0.0, 1.0, 0)
    solo = [ContinuousBatcher(e, eos_ids=eos).run([Request(p, max_new_tokens=20)])[0].tolist() for p in others]
    cb = ContinuousBatcher(e, eos_ids=eos)
    beam = Request(ids, max_new_tokens=N_NEW, num_beams=B, num_return=N_RET, length_penalty=-0.5)
    outs = cb.run([Request(others[0], max_new_tokens=20), beam, Request(others[1], max_new_tokens=20)])
    assert [outs[0].tolist(), outs[2].tolist()] == solo
    want = ranked(-0.5)
    assert [o.tolist() for o in beam.outputs] == [h["tokens"] for h in want] and outs[1].tolist() == want[0]["tokens"]
    assert beam.cumulative_logprobs == [h["cum"] for h in want] and beam.finish_reasons == [h["finish_reason"] for h in want]
    total, free = e.kv_pool_info()
    assert free == total


def test_without_num_beams_nothing_changes(case):
    cfg, model, ids, eos, _ = case
    x = torch.from_numpy(np.stack([_prompt(cfg, 30, seed=8), _prompt(cfg, 30, seed=9)]).astype(np.int64))
    after = [model.generate(input_ids=x, max_new_tokens=24, eos_token_id=[], continuous=c).tolist() for c in (False, True)]
    _, fresh = _model()
    try:
        before = [fresh.generate(input_ids=x, max_new_tokens=24, eos_token_id=[], continuous=c).tolist() for c in (False, True)]
    finally:
        fresh.engine.close()
    assert after == before and after[0] == after[1]
