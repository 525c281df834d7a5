"""Streaming through the server on the real tiny engine: for every request the joined `delta.content` per index equals the
unstreamed `message.content` of the same request, with the same finish_reason / stop_reason, the usage chunk equals `usage`, the streamed
logprob entries equal the unstreamed ones; and modeling.generate(streamer=) puts exactly the new tokens it returns."""
import json

import pytest

pytestmark = pytest.mark.gpu

fastapi = pytest.importorskip("fastapi")
from fastapi.testclient import TestClient  # noqa: E402

PROMPT = "Extract the text content from this image."
N_NEW = 40


@pytest.fixture(scope="module")
def served():
    from dots_ocr_amd.config import DotsConfig
    from dots_ocr_amd.image_utils import PILimage_to_base64
    from dots_ocr_amd.modeling import DotsOcrHipForCausalLM
    from dots_ocr_amd.processing import DotsOcrProcessor
    from dots_ocr_amd.server import create_app
    from dots_ocr_amd.synthetic import synth_page
    from dots_ocr_amd.weights import random_state_dict
    cfg = DotsConfig.tiny(layers=2, v_layers=2)
    model = DotsOcrHipForCausalLM(cfg, random_state_dict(cfg, seed=11), device=0, max_batch=4, max_seq_len=1024, max_patches=4096)
    proc = DotsOcrProcessor(cfg, engine=model.engine)
    page = synth_page(0, (224, 168))
    app = create_app(model, proc, model_name="model", max_batch=4, max_wait_ms=20)
    with TestClient(app) as c:
        app.state.worker.chunk = 8                          # several chunks inside 40 tokens
        yield c, model, proc, page, PILimage_to_base64(page)
    model.engine.close()


def _body(url, **kw):
    body = {"model": "model", "messages": [{"role": "user", "content": [
        {"type": "image_url", "image_url": {"url": url}}, {"type": "text", "text": f"<|img|><|imgpad|><|endofimg|>{PROMPT}"}]}],
        "max_completion_tokens": N_NEW, "temperature": 1.0, "top_p": 1.0, "seed": 7}
    body.update(kw)
    return body


def _chunks(r):
    assert r.status_code == 200 and r.headers["content-type"].startswith("text/event-stream"), r.text
    blocks = [b for b in r.text.split("\n\n") if b.strip()]
    assert all(b.startswith("data: ") for b in blocks) and blocks[-1] == "data: [DONE]"
    return [json.loads(b[6:]) for b in blocks[:-1]]


def _compare(c, url, n=1, least=9, **kw):
    """the same request unstreamed and streamed; -> (unstreamed response, streamed chunks)"""
    if n > 1:
        kw["n"] = n
    plain = c.post("/v1/chat/completions", json=_body(url, **kw))
    assert plain.status_code == 200, plain.text
    plain = plain.json()
    chunks = _chunks(c.post("/v1/chat/completions", json=_body(url, stream=True, stream_options={"include_usage": True}, **kw)))
    assert [ch["choices"][0]["delta"] for ch in chunks[:n]] == [{"role": "assistant", "content": ""}] * n
    assert chunks[-1]["choices"] == [] and chunks[-1]["usage"] == plain["usage"]
    for i in range(n):
        mine = [ch["choices"][0] for ch in chunks[n:-1] if ch["choices"][0]["index"] == i]
        want = plain["choices"][i]
        assert "".join(m["delta"].get("content", "") for m in mine) == want["message"]["content"], i
        assert mine[-1]["delta"] == {} and mine[-1]["finish_reason"] == want["finish_reason"]
        assert mine[-1].get("stop_reason") == want.get("stop_reason") and ("stop_reason" in mine[-1]) == ("stop_reason" in want)
        assert len(mine) > (2 if least > 8 else 1)                                       # it did arrive in pieces
    assert plain["usage"]["completion_tokens"] >= least * n
    return plain, chunks


def test_seeded_sampled_request_streams_its_unstreamed_text(served):
    c, _, _, _, url = served
    _compare(c, url)


def test_two_choices_stream_interleaved_by_index(served):
    c, _, _, _, url = served
    plain, chunks = _compare(c, url, n=2)
    assert plain["choices"][0]["message"]["content"] != plain["choices"][1]["message"]["content"]
    order = [ch["choices"][0]["index"] for ch in chunks[2:-1]]
    assert order != sorted(order)                                                         # interleaved, not one after the other


def test_stop_string_request(served):
    c, _, _, _, url = served
    # the stop string comes from the row's own unstopped output: an ASCII character (one byte, one token of the byte-level vocabulary,
    # control characters included) that first occurs behind the head of the text
    seed = stop = None
    for seed in range(7, 23):
        base = c.post("/v1/chat/completions", json=_body(url, seed=seed)).json()["choices"][0]["message"]["content"]
        stop = next((ch for ch in base[2:] if ord(ch) < 128 and ch not in base[:2]), None)
        if stop is not None:
            break
    assert stop is not None, "no seeded output holds an ASCII character behind its head: a test error, choose other seeds"
    for include in (False, True):
        plain, _ = _compare(c, url, least=1, seed=seed, stop=[stop], include_stop_str_in_output=include)
        ch = plain["choices"][0]
        assert ch["finish_reason"] == "stop" and ch["stop_reason"] == stop
        assert ch["message"]["content"].endswith(stop) == include and len(ch["message"]["content"]) < len(base)


def test_logprob_entries_arrive_with_their_tokens(served):
    c, _, _, _, url = served
    plain, chunks = _compare(c, url, logprobs=True, top_logprobs=2)
    got = [e for ch in chunks[1:-1] if "logprobs" in ch["choices"][0] for e in ch["choices"][0]["logprobs"]["content"]]
    want = plain["choices"][0]["logprobs"]["content"]
    assert got == want and len(want) == plain["usage"]["completion_tokens"] and all(len(e["top_logprobs"]) == 2 for e in want)


def test_generate_with_a_streamer(served):
    import torch
    _, model, proc, page, _ = served

    class Streamer:
        def __init__(self):
            self.puts, self.ended = [], 0

        def put(self, ids):
            self.puts.append(torch.as_tensor(ids).reshape(-1).tolist())

        def end(self):
            self.ended += 1
    messages = [{"role": "user", "content": [{"type": "image", "image": page}, {"type": "text", "text": PROMPT}]}]
    text = proc.apply_chat_template(messages, tokenize=False, add_generation_prompt=True)
    inputs = proc(text=[text], images=[page], padding=True, return_tensors="pt").to("cuda")
    T = inputs.input_ids.shape[1]
    want = model.generate(**inputs, max_new_tokens=N_NEW)[0, T:].tolist()
    st = Streamer()
    out = model.generate(**inputs, max_new_tokens=N_NEW, streamer=st)
    assert out[0, T:].tolist() == want
    assert st.ended == 1 and st.puts[0] == inputs.input_ids[0].tolist() and len(st.puts) > 3
    new = [t for p in st.puts[1:] for t in p]
    pad = model.config.pad_token_id
    assert new == [t for t in want[:len(new)]] and all(t == pad for t in want[len(new):])     # the ids put after the prompt are the new tokens
    two = {k: (torch.cat([v, v]) if k in ("input_ids", "attention_mask") else v) for k, v in inputs.items()}
    for bad in (dict(num_return_sequences=2), dict(num_beams=2), dict(two)):
        with pytest.raises(ValueError):
            model.generate(**{**inputs, **bad}, max_new_tokens=4, streamer=Streamer())
