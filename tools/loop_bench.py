#!/usr/bin/env python3
"""Decode-step time and launch listing with and without the loop guard (profiles/loop_guard.txt).

    python tools/loop_bench.py --loop 1 [--rows 64] [--steps 256] [--reps 5]
        every row sampled under its own seed and carrying the default LoopRule (periods 1 .. 512, 4 repeats, 256 tokens): the check runs
        behind every commit — 512 threads of the stage's workgroup read one earlier id and update one counter each — and never fires
    python tools/loop_bench.py --loop 0
        the same rows without a rule.  This leg uses no call of the feature, so it also runs against the parent commit's library
        (DOTS_OCR_LIB=/path/to/libdots_ocr_hip.so): that run is the baseline.  Alternate the commands in one session
    DOTS_OCR_NO_GRAPH=1 rocprofv3 --kernel-trace --stats -d <dir> -- python tools/loop_bench.py --loop {0,1} --steps 1 --reps 1
        the kernels of one eager step of each leg: the two listings must name the same kernels the same number of times (the --loop 1 leg
        adds the rule's setter and reset kernels outside the step)

Workload: the full-size model with seeded random weights, `rows` text-only prompts of 32 tokens, temperature 1, no EOS.  Per repetition
`steps` decode steps in captured chunks of 16 between two stream synchronises, host clock; one JSON line with the median and the spread
(min, max) of the time per step over the repetitions, after one untimed round.  The tokens of the two legs must be the same (the rule
never fires on these rows): the line carries their digest.
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loop", type=int, default=1, help="1: every row carries the default LoopRule, 0: none does")
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=16)
    ap.add_argument("--tiny", action="store_true", help="tiny dimensions: a rehearsal of the plumbing, not a measurement")
    a = ap.parse_args()
    import torch
    from dots_ocr_amd.config import DotsConfig
    from dots_ocr_amd.engine import Engine, SamplingParams
    from dots_ocr_amd.weights import random_state_dict
    assert torch.cuda.is_available(), "loop_bench needs a GPU"
    cfg = DotsConfig.tiny(layers=2, v_layers=2) if a.tiny else DotsConfig()
    L, rows, steps = 32, a.rows, a.steps
    eng = Engine(cfg, max_batch=rows, max_seq_len=L + steps + 80, max_patches=1024, max_prefill_tokens=rows * L + 64)
    eng.load_state_dict(random_state_dict(cfg, seed=0, threads=16))
    g = np.random.default_rng(3)
    ids = g.integers(1000, 50000 if not a.tiny else cfg.vocab_size - 8, rows * L).astype(np.int32)
    rule = None
    if a.loop:
        from dots_ocr_amd.loop_guard import LoopRule
        rule = LoopRule()

    def run():
        eng.set_sampling(0.0, 1.0, 0)
        eng.slots_reset()
        eng.set_eos([])
        for s in range(rows):
            eng.set_row_sampling(s, SamplingParams(temperature=1.0, top_p=0.95, seed=100 + s))
            if rule is not None:
                eng.set_row_loop(s, rule)
        eng.slots_prefill(list(range(rows)), ids, [L] * rows, [steps + a.chunk + 16] * rows)     # the prefill's token, the warm chunk, the timed steps, and room
        eng.slots_decode(a.chunk if steps >= a.chunk else 1)                   # the captured step of this shape exists before the clock starts
        eng.synchronize()
        t0 = time.perf_counter()
        done = 0
        while done < steps:
            n = min(a.chunk, steps - done)
            eng.slots_decode(n)
            done += n
        eng.synchronize()
        dt = time.perf_counter() - t0
        fin, lens = eng.slots_poll()
        assert all(fin[s] == 0 for s in range(rows)), "a row finished inside the timed window"
        toks = [eng.slot_read(s, int(lens[s])).tolist() for s in range(rows)]
        return dt * 1e3 / steps, toks

    _, tokens = run()                                      # untimed: code objects, graphs, allocations
    per_step = []
    for _ in range(a.reps):
        ms, toks = run()
        assert toks == tokens
        per_step.append(ms)
    import hashlib
    digest = hashlib.sha256(np.asarray(tokens, np.int32).tobytes()).hexdigest()[:16]
    print(json.dumps({"leg": "loop" if a.loop else "plain", "rows": rows, "steps": steps, "reps": a.reps, "tiny": bool(a.tiny),
                      "ms_per_step": {"median": round(statistics.median(per_step), 4), "min": round(min(per_step), 4), "max": round(max(per_step), 4)},
                      "tokens_sha256": digest}), flush=True)


if __name__ == "__main__":
    main()
