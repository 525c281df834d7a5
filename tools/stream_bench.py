#!/usr/bin/env python3
"""Streaming a page's tokens as they are generated (profiles/streaming.txt).

    python tools/stream_bench.py [--slots 8 64] [--new 1024] [--chunk 16] [--reps 3] [--tiny]

Workload: the bench's synthetic A4 page through the processor with the layout prompt, full-size model with seeded random weights, one
request per slot (towers in groups of 8), `new` tokens each, no EOS.  Host clock, one untimed round first, legs alternating.

  (a) arrive    time from submission to the first delivered token and to the last, per request: streamed (Request(stream=): the callback's
                first call / its finished call) against unstreamed (the request's report is the first anything arrives).
  (b) drain     one Engine.slots_drain over every row (tokens + logprob entries, top 5) against what the parent commit offers for the same
                deltas: slots_poll, then slot_read + row_logprobs per row.  Both after the same decode chunks of the same rows.
  (c) decode    tokens per second of the whole run with every row streaming against none (the same runs as (a)).

One JSON line per slot count."""
import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np  # noqa: E402


def _stat(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--new", type=int, default=1024)
    ap.add_argument("--chunk", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--drain-chunks", type=int, default=24, help="decode chunks timed per leg of (b)")
    ap.add_argument("--tiny", action="store_true", help="tiny dimensions and a small page: a rehearsal of the plumbing, not a measurement")
    a = ap.parse_args()
    import torch
    from dots_ocr_amd.config import DotsConfig
    from dots_ocr_amd.engine import Engine
    from dots_ocr_amd.processing import DotsOcrProcessor
    from dots_ocr_amd.prompts import dict_promptmode_to_prompt
    from dots_ocr_amd.scheduler import ContinuousBatcher, Request
    from dots_ocr_amd.synthetic import A4_200DPI, synth_page
    from dots_ocr_amd.weights import random_state_dict
    assert torch.cuda.is_available(), "stream_bench needs a GPU"
    cfg = DotsConfig.tiny(layers=2, v_layers=2) if a.tiny else DotsConfig()
    page = synth_page(0, (224, 168) if a.tiny else A4_200DPI)
    proc = DotsOcrProcessor(cfg)
    messages = [{"role": "user", "content": [{"type": "image", "image": page}, {"type": "text", "text": dict_promptmode_to_prompt["prompt_layout_all_en"]}]}]
    inputs = proc(text=[proc.apply_chat_template(messages, tokenize=False, add_generation_prompt=True)], images=[page], padding=True, return_tensors="pt")
    pv = inputs["pixel_values"].float().contiguous().cuda()          # resident: an admission packs its group's pixels on the device
    grid = inputs["image_grid_thw"].numpy().astype(np.int64)
    P = inputs["input_ids"][0].numpy().astype(np.int32)
    group = 8
    sd = random_state_dict(cfg, seed=0, threads=16)
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None
    except OSError:
        commit = None
    for slots in a.slots:
        eng = Engine(cfg, max_batch=slots, max_seq_len=len(P) + a.new + 128, max_patches=group * pv.shape[0] + 64, max_prefill_tokens=group * len(P) + 64)
        eng.load_state_dict(sd)
        eng.set_sampling(0.0, 1.0, 0)

        def run(streamed, lp=None):
            """every slot one request; -> (first-token ms per request, last-token ms per request, tokens per second of the run)"""
            first, last = {}, {}
            t0 = [0.0]

            def on(rid, index, toks, entries, finished):
                now = (time.perf_counter() - t0[0]) * 1e3
                if len(toks):
                    first.setdefault(rid, now)
                if finished:
                    last[rid] = now
            cb = ContinuousBatcher(eng, eos_ids=(), chunk=a.chunk, admit_group=group, prefetch=0)
            reqs = [Request(P, pv, grid, a.new, logprobs=lp, stream=on if streamed else None) for _ in range(slots)]
            eng.synchronize()
            t0[0] = time.perf_counter()
            ids = [cb.submit(r) for r in reqs]
            n = 0
            while not cb.idle:
                for rid, _, toks in cb.step():
                    now = (time.perf_counter() - t0[0]) * 1e3
                    n += len(toks)
                    if not streamed:                                   # the report is the first the caller sees of it
                        first[rid] = last[rid] = now
            wall = time.perf_counter() - t0[0]
            assert n == slots * a.new and sorted(first) == sorted(last) == ids
            return [first[i] for i in ids], [last[i] for i in ids], n / wall

        def drain_leg(streamed):
            """every slot running with logprobs (top 5); after each of drain_chunks decode chunks the rows' deltas are fetched: one
            slots_drain, or slots_poll + slot_read + row_logprobs per row.  -> ms per fetch"""
            cb = ContinuousBatcher(eng, eos_ids=(), chunk=a.chunk, admit_group=group, prefetch=0)
            for _ in range(slots):
                cb.submit(Request(P, pv, grid, a.new, logprobs=5, stream=(lambda *x: None) if streamed else None))
            while len(cb.running) < slots:
                cb.step()
            if streamed:
                eng.slots_drain()
            _, prev = eng.slots_poll()
            prev = prev.copy()
            ms, got = [], 0
            for _ in range(a.drain_chunks):
                eng.slots_decode(a.chunk)
                eng.synchronize()
                t = time.perf_counter()
                if streamed:
                    _, lens, deltas = eng.slots_drain()
                    got += sum(len(d[0]) for d in deltas.values())
                else:
                    _, lens = eng.slots_poll()
                    for s in range(slots):
                        m = int(lens[s] - prev[s])
                        toks = eng.slot_read(s, int(lens[s]))[int(prev[s]):]
                        eng.row_logprobs(s, m, pos0=int(prev[s]))
                        got += len(toks)
                ms.append((time.perf_counter() - t) * 1e3)
                prev = lens.copy()
            assert got == slots * a.chunk * a.drain_chunks
            eng.slots_reset()
            return ms

        run(True)                                                      # the untimed round of each leg
        run(False)
        t = {"s_first": [], "s_last": [], "u_last": [], "s_tps": [], "u_tps": []}
        for _ in range(a.reps):                                        # alternating: every leg sees the same neighbours on the machine
            f, l, tps = run(True)
            t["s_first"] += f; t["s_last"] += l; t["s_tps"].append(tps)
            f, l, tps = run(False)
            t["u_last"] += l; t["u_tps"].append(tps)
        d = {"drain": [], "per_row": []}
        drain_leg(True); drain_leg(False)
        for _ in range(a.reps):
            d["drain"] += drain_leg(True)
            d["per_row"] += drain_leg(False)
        print(json.dumps({
            "slots": slots, "new_tokens": a.new, "chunk": a.chunk, "reps": a.reps, "prompt_tokens": int(len(P)), "patches": int(pv.shape[0]), "tiny": a.tiny,
            "a_streamed_first_token_ms": _stat(t["s_first"]), "a_streamed_last_token_ms": _stat(t["s_last"]), "a_unstreamed_arrive_ms": _stat(t["u_last"]),
            "b_drain_ms": _stat(d["drain"]), "b_poll_read_logprobs_per_row_ms": _stat(d["per_row"]),
            "b_per_row_over_drain": round(statistics.median(d["per_row"]) / statistics.median(d["drain"]), 2),
            "c_tokens_per_s_streaming": _stat(t["s_tps"]), "c_tokens_per_s_not_streaming": _stat(t["u_tps"]),
            "c_streaming_over_not": round(statistics.median(t["s_tps"]) / statistics.median(t["u_tps"]), 4), "commit": commit}), flush=True)
        eng.close()


if __name__ == "__main__":
    main()
