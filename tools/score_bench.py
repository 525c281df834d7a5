#!/usr/bin/env python3
"""Scoring given tokens on a page: one score request against sequential forcing (profiles/score.txt).

    python tools/score_bench.py [--k 1 4 8] [--tokens 64 512] [--reps 5] [--dpi 200|300] [--kv-cache-dtype bf16|fp8] [--tiny]

Workload: one synthetic A4 page through the processor with the layout prompt, full-size model with seeded random weights, k candidate
answers of n random text tokens each scored behind the prompt.  Two legs on the same engine with 8 slots, alternating, `reps`
repetitions after one untimed round of each, host clock:

  score    one Request(score=[...]) through ContinuousBatcher.run: one tower, one prefill of the prompt, one fork, one
           Engine.slots_score — ceil(k (n + 1) / max_batch) passes of the layer loop, each with an lm_head and a logprob stage.
  forcing  what the parent commit offers: k independent sequences, each with the whole prompt and the page's pixels (k towers and k
           prefills in one admission), logprobs on, then one slots_decode(1) per token with a logit rule that allows the one given id on
           every row, and row_logprobs at the end.  n decode steps of k rows.

Both return the same numbers where they overlap: entry j of a candidate is position j of its forced row, bit for bit on the decode side
(tests/test_score_gpu.py checks that on one engine; here the forcing leg's first token comes from a prefill's logits, so it is compared
at a tolerance and reported).  One JSON line per (k, n).
"""
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
    ap.add_argument("--k", type=int, nargs="+", default=[1, 4, 8])
    ap.add_argument("--tokens", type=int, nargs="+", default=[64, 512])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--top-n", type=int, default=0)
    ap.add_argument("--dpi", type=int, choices=[200, 300], default=200, help="the A4 page's resolution: 1654 x 2339 or 2480 x 3508 pixels")
    ap.add_argument("--kv-cache-dtype", choices=["bf16", "fp8"], default="bf16")
    ap.add_argument("--tiny", action="store_true", help="tiny dimensions and a small page: a rehearsal of the plumbing, not a measurement")
    a = ap.parse_args()
    import torch
    from dots_ocr_amd.config import DotsConfig
    from dots_ocr_amd.engine import Engine, LogitRules
    from dots_ocr_amd.processing import DotsOcrProcessor
    from dots_ocr_amd.prompts import dict_promptmode_to_prompt
    from dots_ocr_amd.scheduler import ContinuousBatcher, Request
    from dots_ocr_amd.synthetic import A4_200DPI, synth_page
    from dots_ocr_amd.weights import random_state_dict
    assert torch.cuda.is_available(), "score_bench needs a GPU"
    cfg = DotsConfig.tiny(layers=2, v_layers=2) if a.tiny else DotsConfig()
    page = synth_page(0, (224, 168) if a.tiny else A4_200DPI if a.dpi == 200 else (2480, 3508))
    proc = DotsOcrProcessor(cfg)
    messages = [{"role": "user", "content": [{"type": "image", "image": page}, {"type": "text", "text": dict_promptmode_to_prompt["prompt_layout_all_en"]}]}]
    inputs = proc(text=[proc.apply_chat_template(messages, tokenize=False, add_generation_prompt=True)], images=[page], padding=True, return_tensors="pt")
    pv = np.ascontiguousarray(inputs["pixel_values"].numpy(), dtype=np.float32)
    grid = inputs["image_grid_thw"].numpy().astype(np.int64)
    P = inputs["input_ids"][0].numpy().astype(np.int32)
    k_max, n_max, slots = max(a.k), max(a.tokens), 8
    assert k_max <= slots
    eng = Engine(cfg, max_batch=slots, max_seq_len=len(P) + n_max + 128, max_patches=k_max * pv.shape[0] + 64, max_prefill_tokens=k_max * len(P) + 64,
                 kv_cache_dtype=a.kv_cache_dtype)
    eng.load_state_dict(random_state_dict(cfg, seed=0, threads=16))
    eng.set_sampling(0.0, 1.0, 0)
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None
    except OSError:
        commit = None
    rng = np.random.default_rng(0)
    hi = min(cfg.vocab_size, 256 if a.tiny else 100000)                # plain text ids: no image token, no EOS
    for n in a.tokens:
        cands_all = [[int(t) for t in rng.integers(0, hi, n)] for _ in range(k_max)]
        for k in a.k:
            cands = cands_all[:k]
            fed = [[int(P[-1])] + c for c in cands]                    # as the server feeds them: every candidate token gets an entry

            def score():
                r = Request(P[:-1], pv, grid, score=fed, score_top_logprobs=a.top_n)
                cb = ContinuousBatcher(eng, eos_ids=(), chunk=16)
                eng.synchronize()
                t0 = time.perf_counter()
                cb.run([r])
                return (time.perf_counter() - t0) * 1e3, [s[0] for s in r.scores_out]

            def forcing():
                eng.slots_reset()
                eng.set_eos([])
                eng.synchronize()
                t0 = time.perf_counter()
                rows = list(range(k))
                for s in rows:
                    eng.set_row_logprobs(s, a.top_n)
                    eng.set_row_logit_rules(s, LogitRules(allowed=(cands[s][0],)))
                eng.vit_forward(np.concatenate([pv] * k), np.concatenate([grid] * k))
                eng.slots_prefill(rows, np.concatenate([P] * k), [len(P)] * k, [n + 1] * k)
                for j in range(1, n):
                    for s in rows:
                        eng.set_row_logit_rules(s, LogitRules(allowed=(cands[s][j],)))
                    eng.slots_decode(1)
                out = [eng.row_logprobs(s, n)[0] for s in rows]
                ms = (time.perf_counter() - t0) * 1e3
                toks = [eng.slot_read(s, n).tolist() for s in rows]
                for s in rows:
                    eng.set_row_logit_rules(s, None)
                    eng.set_row_logprobs(s, None)
                eng.slots_reset()
                assert toks == cands, "the forcing did not hold"
                return ms, out

            _, got = score()                                           # the untimed round
            _, want = forcing()
            # entry 0 of the forcing leg comes from the prefill's logits, the score's from a decode pass: two valid evaluations
            diff = max(float(np.abs(g.astype(np.float64) - w.astype(np.float64)).max()) for g, w in zip(got, want))
            t = {"score": [], "forcing": []}
            for _ in range(a.reps):                                    # alternating: every leg sees the same neighbours on the machine
                t["score"].append(score()[0])
                t["forcing"].append(forcing()[0])
            med = {name: statistics.median(v) for name, v in t.items()}
            rows_fed = k * (n + 1)
            print(json.dumps({"k": k, "tokens": n, "dpi": a.dpi, "prompt_tokens": int(len(P)), "patches": int(pv.shape[0]), "slots": slots, "top_n": a.top_n,
                              "kv_cache_dtype": a.kv_cache_dtype, "reps": a.reps, "score_ms": _stat(t["score"]), "forcing_ms": _stat(t["forcing"]),
                              "score_passes": -(-rows_fed // slots), "forcing_steps": n - 1, "forcing_over_score": round(med["forcing"] / med["score"], 2),
                              "max_abs_logprob_difference": round(diff, 5), "commit": commit}), flush=True)


if __name__ == "__main__":
    main()
