#!/usr/bin/env python3
"""The logprob stage at the real vocabulary (V = 151 936; profiles/logprobs.txt).

    python tools/logprobs_bench.py [--rows 1 8 64] [--top-n 0 5 20] [--iters 200] [--loop-steps 64]
        per (row count, top_n), mean time of one stage (HIP events around `iters` replays after a warm-up, one process):
          stage    both kernels (logprob_partial_kernel + logprob_final_kernel), every row on
          partial  logprob_partial_kernel alone
          final    logprob_final_kernel alone
        then, unless --loop-steps 0, the running decode loop: 64 occupied slots of a model with the real vocabulary and tiny layers
        (random weights), `loop-steps` captured decode steps per measurement with every row off and with every row at top_n = 20;
        the difference is the step time the stage adds inside the loop.
Logits: a seeded N(0, 2) background with 64 planted tokens in [8, 14] per row.  One JSON line per measurement on stdout.
"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np  # noqa: E402

V = 151936


def loop_time(steps, reps):
    """ms per decode step of 64 slots, logprobs off and on (every row, top_n = 20), best of `reps` chunks each"""
    from dots_ocr_amd.config import DotsConfig
    from dots_ocr_amd.engine import Engine
    from dots_ocr_amd.weights import random_state_dict
    cfg = DotsConfig.tiny(layers=2, v_layers=1, vocab=V)
    e = Engine(cfg, max_batch=64, max_seq_len=1024, max_patches=256, max_prefill_tokens=64 * 32)
    e.load_state_dict(random_state_dict(cfg, seed=3))
    rng = np.random.default_rng(1)
    prompts = [rng.integers(0, V - 8, 24).astype(np.int32) for _ in range(64)]
    out = {}
    for name, top_n in (("off", None), ("on", 20), ("off_again", None)):
        e.slots_reset()
        e.set_eos([])
        for s in range(64):
            e.set_row_logprobs(s, top_n)
        e.slots_prefill(list(range(64)), np.concatenate(prompts), [24] * 64, [steps * (reps + 1) + 2] * 64)
        e.slots_decode(steps)                                   # capture + warm-up
        e.synchronize()
        best = float("inf")
        for _ in range(reps):
            t0 = time.perf_counter()
            e.slots_decode(steps)
            e.synchronize()
            best = min(best, (time.perf_counter() - t0) * 1e3 / steps)
        out[name] = best
    e.slots_reset()
    e.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--top-n", type=int, nargs="+", default=[0, 5, 20])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--loop-steps", type=int, default=64)
    ap.add_argument("--loop-reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    from dots_ocr_amd.config import DotsConfig
    from dots_ocr_amd.engine import Engine
    eng = Engine(DotsConfig.tiny(), max_batch=4, max_seq_len=512, max_patches=256, max_prefill_tokens=256)
    rng = np.random.default_rng(0)
    B_max = max(a.rows)
    logits = rng.normal(0.0, 2.0, (B_max, V)).astype(np.float32)
    for b in range(B_max):
        logits[b, rng.choice(V, 64, replace=False)] = rng.uniform(8.0, 14.0, 64)
    d_l = torch.from_numpy(logits).cuda()
    torch.cuda.synchronize()
    for B in a.rows:
        for n in a.top_n:
            for name, which in (("stage", 0), ("partial", 1), ("final", 2)):
                ms = eng.bench_logprobs(d_l.data_ptr(), B, V, V, [n] * B, which, a.iters)
                print(json.dumps({"rows": B, "V": V, "top_n": n, "kernels": name, "us": round(ms * 1e3, 2), "iters": a.iters}), flush=True)
    eng.close()
    if a.loop_steps > 0:
        t = loop_time(a.loop_steps, a.loop_reps)
        print(json.dumps({"loop": "64 slots, tiny layers, V = 151936", "steps": a.loop_steps, "ms_per_step_off": round(t["off"], 4),
                          "ms_per_step_top20": round(t["on"], 4), "ms_per_step_off_again": round(t["off_again"], 4),
                          "extra_us_per_step": round((t["on"] - min(t["off"], t["off_again"])) * 1e3, 1)}), flush=True)


if __name__ == "__main__":
    main()
