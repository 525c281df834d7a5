"""generate() gives a call's row settings to the rows of a static batch and to the requests of the continuous path from one feature table
(dots_ocr_amd/row_features.py): both paths must return the same ids for the same call, and nothing may stay on a row afterwards.  This is
the only check that runs the static path's set and clear loops.

Tiny random model, three text-only prompts of 8, 10 and 12 tokens padded with an attention mask, 16 new tokens; the token bytes are the
synthetic table of test_stop_strings_gpu.py.  Every call is made once, in a module fixture, in the order a user would make them."""
import numpy as np
import pytest
import torch

from dots_ocr_amd.config import DotsConfig
from dots_ocr_amd.weights import random_state_dict
from test_stop_strings_gpu import TOKS, V

pytestmark = pytest.mark.gpu

NEW = 16
SAMPLED = dict(do_sample=True, top_k=8, temperature=0.8, seed=3, repetition_penalty=1.1)
CASES = ("sampled", "sampled+rules", "ngram", "stop_strings")


@pytest.fixture(scope="module")
def runs():
    from dots_ocr_amd.modeling import DotsOcrHipForCausalLM
    cfg = DotsConfig.tiny(layers=3, v_layers=3, vocab=V)
    model = DotsOcrHipForCausalLM(cfg, random_state_dict(cfg, seed=11), max_batch=4, max_seq_len=640, max_patches=4096)
    model.engine.set_token_bytes(TOKS)
    g = np.random.default_rng(31)
    lens = (8, 10, 12)
    ids = torch.full((3, max(lens)), int(cfg.pad_token_id), dtype=torch.long)
    mask = torch.zeros((3, max(lens)), dtype=torch.long)
    for b, n in enumerate(lens):
        ids[b, :n] = torch.from_numpy(g.integers(0, V - 8, n))
        mask[b, :n] = 1

    def both(**kw):
        return tuple(model.generate(ids, mask, max_new_tokens=NEW, continuous=c, **kw) for c in (False, True))

    out = {"T": ids.shape[1], "pad": int(cfg.pad_token_id)}
    out["before"] = both()
    greedy = out["before"][0][:, ids.shape[1]:]
    out["banned"] = sorted({int(t) for t in greedy[:, 0]})
    # stop ids and a stop string from what row 0 would generate anyway: they have something to end
    out["stop_ids"] = [int(greedy[0, 5])]
    i = next(i for i in range(4, NEW - 1) if TOKS[int(greedy[0, i])] and TOKS[int(greedy[0, i + 1])])
    out["stop_string"] = (TOKS[int(greedy[0, i])] + TOKS[int(greedy[0, i + 1])]).decode()
    out["stop_by"] = i + 2
    out["sampled"] = both(**SAMPLED)
    out["sampled+rules"] = both(**SAMPLED, logit_bias={t: float("-inf") for t in out["banned"]}, stop_token_ids=out["stop_ids"], min_tokens=2)
    out["ngram"] = both(no_repeat_ngram_size=2)
    out["stop_strings"] = both(stop_strings=[out["stop_string"]])
    out["after"] = both()
    yield out
    model.engine.close()


def _rows(out, res):
    """the new tokens of every row without the pads behind them (the pad id is an EOS id: a final EOS goes with them)"""
    rows = []
    for r in res[:, out["T"]:].tolist():
        while r and r[-1] == out["pad"]:
            r.pop()
        rows.append(r)
    return rows


@pytest.mark.parametrize("case", CASES)
def test_the_static_and_the_continuous_path_return_the_same_ids(runs, case):
    static, continuous = runs[case]
    assert static.shape == continuous.shape and torch.equal(static, continuous)


def test_the_settings_reached_the_rows(runs):
    """each case did something: equal ids on both paths are not two runs that both ignored the setting"""
    greedy = runs["before"][0]
    for case in CASES:
        assert not torch.equal(runs[case][0], greedy), case
    for r in _rows(runs, runs["sampled+rules"][0]):
        assert r[0] not in runs["banned"] and not set(r[:2]) & set(runs["stop_ids"])
        assert all(t not in runs["stop_ids"] for t in r[:-1])                   # a stop id ends its row
    for r in _rows(runs, runs["ngram"][0]):
        pairs = list(zip(r, r[1:]))
        assert len(set(pairs)) == len(pairs)
    assert len(_rows(runs, runs["stop_strings"][0])[0]) <= runs["stop_by"]


def test_nothing_stays_on_a_row(runs):
    for before, after in zip(runs["before"], runs["after"]):
        assert torch.equal(before, after)
    assert torch.equal(runs["before"][0], runs["before"][1])
