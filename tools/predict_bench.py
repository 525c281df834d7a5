#!/usr/bin/env python3
"""What a prediction buys a speculating decode, and what the second drafter costs (profiles/predicted_outputs.txt).

    python tools/predict_bench.py [--slots 8] [--k 3] [--prompt 5002] [--new 256] [--repeats 5] [--configs NAME ..] [--tiny]

Full-size language model with seeded random weights (the vision tower, which no text-only prompt touches, is cut to one block), one
engine, `slots` pages of `prompt` tokens each (5002 = the bench's A4 page) decoding `new` tokens in captured chunks of 16 steps, as the
scheduler runs them.  The reference tokens T come from an unspeculated run; every configuration must reproduce them exactly.

    unspeculated    k = 0
    ngram           n-gram speculation alone: the parent commit's behaviour, the baseline
    perfect         every row's own T as its prediction: the ceiling
    replaced_5 / replaced_20   T with 5 % / 20 % of the tokens replaced by ids T never holds
    moved           T cut into spans of 48 tokens, adjacent spans exchanged (regions in another order)
    scaffold        a fixed run of 6 tokens inserted into T every 32 tokens (plain text against JSON-wrapped output)
    never           every slot holds a max_seq_len-long prediction of ids T never holds: the drafter searches and never finds — against
                    `ngram` this is the cost of the launch itself

The configurations of one repeat run one after the other, so that they alternate; reported per configuration: the median over the
repeats of the wall time from the first decode chunk to the poll that sees every row finished (min and max beside it), ms per launched
step, tokens per row step (from dots_spec_stats), ms per page = wall / slots, and the accepted / drafted prediction tokens.  One JSON
line per configuration on stdout, then a table.  With DOTS_OCR_LIB set the same script measures another build of the library (the
parent commit's, for the configurations it knows: --configs unspeculated ngram)."""
import argparse
import dataclasses
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np  # noqa: E402

CONFIGS = ("unspeculated", "ngram", "perfect", "replaced_5", "replaced_20", "moved", "scaffold", "never")


def variants(T, free, rng, seq):
    def replaced(share):
        out = list(T)
        for i in rng.choice(len(T), int(len(T) * share), replace=False):
            out[int(i)] = int(free[int(i) % len(free)])
        return out
    spans = [T[i:i + 48] for i in range(0, len(T), 48)]
    for i in range(0, len(spans) - 1, 2):
        spans[i], spans[i + 1] = spans[i + 1], spans[i]
    scaffold = []
    for i in range(0, len(T), 32):
        scaffold += [int(t) for t in free[:6]] + T[i:i + 32]
    return {"perfect": list(T), "replaced_5": replaced(0.05), "replaced_20": replaced(0.20), "moved": [t for s in spans for t in s],
            "scaffold": scaffold, "never": [int(free[i % len(free)]) for i in range(seq)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=8)
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--prompt", type=int, default=5002)
    ap.add_argument("--new", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--configs", nargs="+", default=list(CONFIGS), choices=CONFIGS)
    ap.add_argument("--tiny", action="store_true", help="the small-dims model (a plumbing check, not a measurement)")
    a = ap.parse_args()
    from dots_ocr_amd.config import DotsConfig
    from dots_ocr_amd.engine import Engine
    from dots_ocr_amd.weights import random_state_dict
    if a.tiny:
        cfg = DotsConfig.tiny(layers=3, v_layers=1)
    else:
        cfg = DotsConfig()
        cfg = dataclasses.replace(cfg, vision=dataclasses.replace(cfg.vision, num_hidden_layers=1))
    S, seq = a.slots, a.prompt + a.new + 64
    eng = Engine(cfg, max_batch=S * (a.k + 1), max_seq_len=seq, max_patches=256, max_prefill_tokens=S * a.prompt)
    eng.load_state_dict(random_state_dict(cfg, seed=0, threads=16))
    eng.set_eos([])
    eng.set_sampling(0.0, 1.0, 0)
    rng = np.random.default_rng(0)
    top = cfg.vocab_size - min(4096, cfg.vocab_size // 8)          # below the special ids
    prompts = [rng.integers(0, top, a.prompt).astype(np.int32) for _ in range(S)]
    slots = list(range(S))
    has_pred = hasattr(eng.lib, "dots_set_row_prediction")

    def run(k, preds=None):
        eng.slots_reset()
        eng.set_speculation(k, 2, 4)
        for b in slots:
            if preds is not None:
                eng.set_row_prediction(b, preds[b])
        eng.slots_prefill(slots, np.concatenate(prompts), [a.prompt] * S, [a.new] * S)
        eng.synchronize()
        launched = 0
        t0 = time.perf_counter()
        while True:
            eng.slots_decode(16)
            launched += 16
            fin, lens = eng.slots_poll()
            if all(fin[b] == 1 for b in slots):
                break
        dt = time.perf_counter() - t0
        toks = [eng.slot_read(b, int(lens[b])).tolist() for b in slots]
        st = [eng.spec_stats(b) for b in slots] if k else [{"steps": a.new - 1, "drafted": 0, "accepted": 0}] * S
        pst = [eng.row_prediction_stats(b) for b in slots] if preds is not None else [{"drafted": 0, "accepted": 0}] * S
        for b in slots:
            eng.slot_release(b)
        return dict(dt=dt, launched=launched, toks=toks, row_steps=sum(s["steps"] for s in st) / S, drafted=sum(s["drafted"] for s in st),
                    accepted=sum(s["accepted"] for s in st), pred_drafted=sum(p["drafted"] for p in pst), pred_accepted=sum(p["accepted"] for p in pst))

    T = run(0)["toks"]
    assert all(len(t) == a.new for t in T)
    made = []
    for b in slots:
        free = np.setdiff1d(np.arange(top), np.asarray(T[b]))
        made.append(variants(T[b], free, np.random.default_rng(100 + b), seq))
    runs = {c: [] for c in a.configs}
    for c in a.configs:                                              # warm-up: every captured step exists before a clock starts
        if c in made[0] and not has_pred:
            raise SystemExit(f"this build of the library takes no prediction: --configs unspeculated ngram")
        run(0 if c == "unspeculated" else a.k, [m[c] for m in made] if c in made[0] else None)
    for _ in range(a.repeats):
        for c in a.configs:
            r = run(0 if c == "unspeculated" else a.k, [m[c] for m in made] if c in made[0] else None)
            assert r["toks"] == T, f"{c}: the run left the reference tokens"
            runs[c].append(r)
    rows = []
    for c in a.configs:
        rs = runs[c]
        dt = statistics.median(r["dt"] for r in rs)
        r0 = rs[0]
        rec = {"config": c, "slots": S, "k": 0 if c == "unspeculated" else a.k, "prompt": a.prompt, "new": a.new, "repeats": a.repeats,
               "wall_ms": round(dt * 1e3, 2), "wall_ms_min_max": [round(min(r["dt"] for r in rs) * 1e3, 2), round(max(r["dt"] for r in rs) * 1e3, 2)],
               "steps_launched": r0["launched"], "ms_per_step": round(dt / r0["launched"] * 1e3, 4), "row_steps": round(r0["row_steps"], 2),
               "tokens_per_row_step": round((a.new - 1) / r0["row_steps"], 3), "ms_per_page": round(dt / S * 1e3, 2),
               "drafted": r0["drafted"], "accepted": r0["accepted"], "pred_drafted": r0["pred_drafted"], "pred_accepted": r0["pred_accepted"]}
        rows.append(rec)
        print(json.dumps(rec), flush=True)
    print()
    print(f"{'config':>13} {'wall ms (min .. max)':>28} {'steps':>6} {'ms/step':>8} {'tok/row step':>12} {'ms/page':>8} {'pred acc/drafted':>17}")
    for r in rows:
        spread = f"{r['wall_ms']:.1f} ({r['wall_ms_min_max'][0]:.1f} .. {r['wall_ms_min_max'][1]:.1f})"
        print(f"{r['config']:>13} {spread:>28} {r['steps_launched']:>6} {r['ms_per_step']:>8.4f} {r['tokens_per_row_step']:>12.3f} {r['ms_per_page']:>8.2f} "
              f"{str(r['pred_accepted']) + ' / ' + str(r['pred_drafted']):>17}")
    eng.close()


if __name__ == "__main__":
    main()
