"""Per-token logprobs on the GPU: the two-kernel stage against numpy fp64 log_softmax at the real vocabulary, and the
engine contract on the tiny model: every committed token gets its value, the top entries follow the arg-max tie rule, a row's values
are bitwise the same alone / in a batch / in any slot / on the static path, and nothing else changes when logprobs are on."""
import numpy as np
import pytest
import torch

from dots_ocr_amd.config import DotsConfig
from dots_ocr_amd.engine import SamplingParams
from dots_ocr_amd.weights import random_state_dict

pytestmark = pytest.mark.gpu

V = 151936
K = 20
CHUNK = ((V + 63) // 64 + 3) // 4 * 4                    # the stage's vocabulary chunk (logprobs.hip lp_chunk_len)


@pytest.fixture(scope="module")
def eng():
    from dots_ocr_amd.engine import Engine
    cfg = DotsConfig.tiny(layers=3, v_layers=3, vocab=1024)
    e = Engine(cfg, max_batch=4, max_seq_len=640, max_patches=4096, max_prefill_tokens=2048)
    e.load_state_dict(random_state_dict(cfg, seed=23))
    yield cfg, e
    e.close()


def _ref(l):
    """numpy fp64 log_softmax and the full (value desc, index asc) order of one fp32 row"""
    x = l.astype(np.float64)
    m = x.max()
    lp = x - (m + np.log(np.exp(x - m).sum()))
    return lp, np.lexsort((np.arange(x.shape[0]), -x))


def _close(got, want):
    return np.all(np.abs(np.asarray(got, np.float64) - want) <= 1e-4 + 1e-5 * np.abs(want))


def _planted(rng, kind):
    l = rng.normal(0.0, 3.0, V).astype(np.float32)
    if kind == "tie_max":                                 # exact ties at the maximum, in different chunks
        l[rng.choice(V, 3, replace=False)] = 30.0
    elif kind == "tie_boundary":                          # 30 equal values straddling chunk boundaries: the 20th place falls among them
        idx = np.concatenate([[c * CHUNK - 1, c * CHUNK] for c in range(3, 63, 4)])
        l[idx] = 25.0
        l[rng.choice(V, 6, replace=False)] = 26.0
    elif kind == "equal":
        l[:] = 0.5
    elif kind == "wide":
        l = rng.uniform(-1e4, 50.0, V).astype(np.float32)
    return l


KINDS = ("noise", "tie_max", "tie_boundary", "equal", "wide")


@pytest.mark.parametrize("B", [1, 8, 64])
def test_op_logprobs_match_numpy(eng, B):
    _, e = eng
    rng = np.random.default_rng(100 + B)
    kinds = [KINDS[(b + B) % len(KINDS)] for b in range(B)]
    L = np.stack([_planted(rng, k) for k in kinds])
    top_n = [(0, 1, 5, 20, -1)[(b * 3 + B) % 5] if B > 1 else 20 for b in range(B)]
    chosen = np.array([int(np.argmax(L[b])) if b % 2 == 0 else int(rng.integers(0, V)) for b in range(B)], np.int32)
    d_l = torch.from_numpy(L).cuda()
    d_c = torch.from_numpy(chosen).cuda()
    tok = torch.full((B,), 7.0, dtype=torch.float32, device="cuda")                # sentinel: rows with top_n = -1 stay untouched
    ids = torch.full((B, K), 7, dtype=torch.int32, device="cuda")
    top = torch.full((B, K), 7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    e.op_logprobs(d_l.data_ptr(), B, V, V, top_n, d_c.data_ptr(), tok.data_ptr(), ids.data_ptr(), top.data_ptr())
    tok, ids, top = tok.cpu().numpy(), ids.cpu().numpy(), top.cpu().numpy()
    for b in range(B):
        n = top_n[b]
        if n < 0:
            assert tok[b] == 7.0 and (ids[b] == 7).all() and (top[b] == 7.0).all()
            continue
        lp, order = _ref(L[b])
        assert _close(tok[b], lp[chosen[b]]), (b, kinds[b], tok[b], lp[chosen[b]])
        assert np.array_equal(ids[b, :n], order[:n]), (b, kinds[b], ids[b, :n], order[:n])
        assert _close(top[b, :n], lp[order[:n]]), (b, kinds[b])
        assert (ids[b, n:] == -1).all() and np.isnan(top[b, n:]).all()
        if kinds[b] == "equal":
            assert _close(tok[b], -np.log(V))
        if b % 2 == 0 and n > 0:                          # the chosen token is the arg max: bitwise its top entry
            assert ids[b, 0] == chosen[b] and tok[b] == top[b, 0]


# ---------------------------------------------------------------------------------------------------- engine

STEPS = 14
LP = [None, 0, 5, 20]
PARAMS = [None, SamplingParams(temperature=0.9, seed=5), SamplingParams(repetition_penalty=3.0), None]


def _prompts(cfg):
    g = np.random.default_rng(7)
    ps = [g.integers(0, cfg.vocab_size - 8, 6 + 3 * b).astype(np.int32) for b in range(4)]
    return np.concatenate(ps), np.array([len(p) for p in ps], np.int32)


def _set_rows(e, lp=LP):
    for b in range(4):
        e.set_row_sampling(b, PARAMS[b])
        e.set_row_logprobs(b, lp[b])


def _clear_rows(e):
    for b in range(4):
        e.set_row_sampling(b, None)
        e.set_row_logprobs(b, None)


def _static_steps(e, packed, lens, lp):
    """static prefill + STEPS eager decode steps: (logits [STEPS + 1, 4, V], tokens [STEPS + 1, 4])"""
    _set_rows(e, lp)
    e.prefill(packed, lens)
    logits, toks = [e.get_logits()], [e.get_last_tokens()]
    for _ in range(STEPS):
        e.decode_step()
        logits.append(e.get_logits())
        toks.append(e.get_last_tokens())
    return np.stack(logits), np.stack(toks)


def _check_row(lp_out, logits, toks, n_top, greedy_plain):
    """the contract for one row: logits [P, V], toks [P] per position"""
    tok_lp, ids, top = lp_out
    flips = 0
    for n in range(len(toks)):
        lp, order = _ref(logits[n])
        t = int(toks[n])
        assert _close(tok_lp[n], lp[t]), (n, tok_lp[n], lp[t])
        assert np.array_equal(ids[n, :n_top], order[:n_top]), n
        assert _close(top[n, :n_top], lp[order[:n_top]]), n
        assert (ids[n, n_top:] == -1).all() and np.isnan(top[n, n_top:]).all()
        if greedy_plain:
            assert t == order[0] and tok_lp[n] == top[n, 0] and ids[n, 0] == t
        if n_top > 0 and t != order[0]:
            assert ids[n, 0] == order[0]                  # the raw arg max, whatever the penalty chose
            flips += 1
    return flips


def test_engine_logprobs_follow_the_contract_on_every_path(eng):
    cfg, e = eng
    packed, lens = _prompts(cfg)
    P = STEPS + 1
    e.set_sampling(0.0, 1.0, 0)
    e.set_eos([])
    try:
        # ---- static, step by step: the numpy reference from the engine's own logits; on vs off changes neither logits nor tokens
        _clear_rows(e)
        l_off, t_off = _static_steps(e, packed, lens, [None] * 4)
        l_on, t_on = _static_steps(e, packed, lens, LP)
        assert np.array_equal(l_on, l_off) and np.array_equal(t_on, t_off)
        static = [e.row_logprobs(b, P) for b in range(4)]
        assert all(len(s[0]) == P for s in static)
        assert np.isnan(static[0][0]).all() and (static[0][1] == -1).all() and np.isnan(static[0][2]).all()
        flips = 0
        for b in (1, 2, 3):
            f = _check_row(static[b], l_on[:, b], t_on[:, b], LP[b], greedy_plain=(b == 3))
            if b == 2:
                flips = f
        assert flips >= 1, "the penalised greedy row never moved off the raw arg max"

        # ---- static dots_generate (captured graphs): bitwise the step-by-step values
        out, olen = e.generate(packed, lens, max_new_tokens=P)
        assert (olen == P).all() and np.array_equal(out.T, t_on)
        for b in range(4):
            g = e.row_logprobs(b, P)
            for x, y in zip(g, static[b]):
                assert np.array_equal(x, y, equal_nan=True), b

        # ---- slots, one step at a time; slot 1 finishes early and keeps its values while the others decode on
        e.slots_reset()
        e.set_eos([])
        _set_rows(e)
        caps = [P, 5, P, P]
        e.slots_prefill([0, 1, 2, 3], packed, lens, caps)
        early = None
        for step in range(STEPS):
            e.slots_decode(1)
            if step == 3:
                early = e.row_logprobs(1, 64)
        toks = [e.slot_read(b, 64) for b in range(4)]
        slot_lp = [e.row_logprobs(b, 64) for b in range(4)]
        assert [len(t) for t in toks] == caps
        for b in range(4):
            assert np.array_equal(toks[b], t_on[:caps[b], b]), b
            for x, y in zip(slot_lp[b], static[b]):
                assert np.array_equal(x, y[:caps[b]], equal_nan=True), b
        assert len(early[0]) == 5
        for x, y in zip(slot_lp[1], early):
            assert np.array_equal(x, y, equal_nan=True)

        # ---- the same slots with logprobs off: the same tokens
        for b in range(4):
            e.slot_release(b)
        _set_rows(e, [None] * 4)
        e.slots_prefill([0, 1, 2, 3], packed, lens, caps)
        e.slots_decode(STEPS)
        assert all(np.array_equal(e.slot_read(b, 64), toks[b]) for b in range(4))
        for b in range(4):
            e.slot_release(b)

        # ---- row 3's request alone, in another slot: bitwise the batch values
        off = int(lens[:3].sum())
        e.set_row_sampling(1, PARAMS[3])
        e.set_row_logprobs(1, LP[3])
        e.slots_prefill([1], packed[off:], [int(lens[3])], [P])
        e.slots_decode(STEPS)
        assert np.array_equal(e.slot_read(1, 64), toks[3])
        for x, y in zip(e.row_logprobs(1, 64), static[3]):
            assert np.array_equal(x, y, equal_nan=True)
        e.slot_release(1)

        # ---- slot 2 served logprobs before; a new request switched on mid-run reads NaN / -1 before the switch
        e.set_row_sampling(2, None)
        e.slots_prefill([2], packed[off:], [int(lens[3])], [P])
        e.slots_decode(3)
        e.set_row_logprobs(2, 5)
        e.slots_decode(3)
        tok_lp, ids, top = e.row_logprobs(2, 64)
        assert len(tok_lp) == 7
        assert np.isnan(tok_lp[:4]).all() and (ids[:4] == -1).all() and np.isnan(top[:4]).all()
        assert np.array_equal(tok_lp[4:], static[3][0][4:7]) and np.array_equal(ids[4:, :5], static[3][1][4:7, :5])
        assert (ids[4:, 5:] == -1).all()
        e.slot_release(2)
    finally:
        e.slots_reset()
        _clear_rows(e)


def test_server_returns_the_engine_values(eng):
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient
    from dots_ocr_amd.processing import DotsOcrProcessor
    from dots_ocr_amd.server import _parse_messages, create_app
    cfg, e = eng

    class Model:
        config = cfg
        engine = e
    proc = DotsOcrProcessor(cfg)
    body = {"model": "model", "messages": [{"role": "user", "content": "Read the page."}], "max_completion_tokens": 8,
            "temperature": 0, "logprobs": True, "top_logprobs": 3}
    app = create_app(Model(), proc, model_name="model", max_batch=4)
    with TestClient(app) as c:
        r = c.post("/v1/chat/completions", json=body)
    assert r.status_code == 200, r.text
    d = r.json()
    content = d["choices"][0]["logprobs"]["content"]
    assert len(content) == d["usage"]["completion_tokens"] >= 1
    # the same prompt straight through the engine
    _, text = _parse_messages(body["messages"], proc)
    ids = proc(text=[text], padding=True, return_tensors="pt")["input_ids"][0].numpy().astype(np.int32)
    e.slots_reset()
    e.set_sampling(0.0, 1.0, 0)
    e.set_eos(cfg.eos_token_ids)
    e.set_row_logprobs(0, 3)
    e.slots_prefill([0], ids, [len(ids)], [8])
    while e.slots_poll()[0][0] != 1:
        e.slots_decode(1)
    toks = e.slot_read(0, 64)
    tok_lp, top_ids, top_lp = e.row_logprobs(0, len(toks))
    e.slot_release(0)
    e.slots_reset()
    assert len(toks) == len(content)
    for n, ent in enumerate(content):
        assert ent["token"] == proc.tokenizer.decode([int(toks[n])], skip_special_tokens=False)
        assert ent["logprob"] == float(tok_lp[n])
        assert [a["logprob"] for a in ent["top_logprobs"]] == [float(x) for x in top_lp[n, :3]]
        assert [a["token"] for a in ent["top_logprobs"]] == [proc.tokenizer.decode([int(t)], skip_special_tokens=False) for t in top_ids[n, :3]]
