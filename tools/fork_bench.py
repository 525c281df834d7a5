#!/usr/bin/env python3
"""Parallel sampling against four posts of the same page (profiles/parallel_sampling.txt).

    python tools/fork_bench.py [--reps 5] [--n 4] [--new-tokens 256] [--seed 1]
        both legs, alternating, in one process: `forked` (one tower, one prefill, Engine.slots_fork, n rows) and `independent` (the
        page's pixels and prompt n times in one group: n towers, n prefills, n rows), after one untimed round of each
    python tools/fork_bench.py --independent
        the independent leg alone.  It uses only calls that exist without slots_fork, so it also runs on the commit before the feature:
        that run is the baseline

Workload: one synthetic A4 page at 200 dpi through the processor (its real prompt), full-size model with seeded random weights, n = 4
sampled sequences (temperature 1.0, top_p 0.95, seeds s .. s + 3), 256 tokens each, no EOS.  Per repetition, host clock from before
the tower is enqueued to a stream synchronise: `first_ms` = until all n first tokens exist, `total_ms` = until all n sequences have
finished.  One JSON line per leg with the median and the spread (min, max) over the repetitions, then whether the two legs gave the
same tokens (they must).
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=4)
    ap.add_argument("--new-tokens", type=int, default=256)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--chunk", type=int, default=16)
    ap.add_argument("--independent", action="store_true", help="the independent leg only (runs without slots_fork)")
    ap.add_argument("--tiny", action="store_true", help="tiny dimensions and a small page: a rehearsal of the plumbing, not a measurement")
    a = ap.parse_args()
    import torch
    from dots_ocr_amd.config import DotsConfig
    from dots_ocr_amd.engine import Engine, SamplingParams
    from dots_ocr_amd.processing import DotsOcrProcessor
    from dots_ocr_amd.synthetic import A4_200DPI, synth_page
    from dots_ocr_amd.weights import random_state_dict
    assert torch.cuda.is_available(), "fork_bench needs a GPU"
    cfg = DotsConfig.tiny(layers=2, v_layers=2) if a.tiny else DotsConfig()
    page = synth_page(0, (224, 168) if a.tiny else A4_200DPI)
    proc = DotsOcrProcessor(cfg)
    messages = [{"role": "user", "content": [{"type": "image", "image": page}, {"type": "text", "text": "Extract the text content from this image."}]}]
    text = proc.apply_chat_template(messages, tokenize=False, add_generation_prompt=True)
    inputs = proc(text=[text], images=[page], padding=True, return_tensors="pt")
    ids = inputs["input_ids"][0].numpy().astype(np.int32)
    pv = np.ascontiguousarray(inputs["pixel_values"].numpy(), dtype=np.float32)
    grid = inputs["image_grid_thw"].numpy().astype(np.int64)
    n, L, new = a.n, len(ids), a.new_tokens
    eng = Engine(cfg, max_batch=n, max_seq_len=L + new + 64, max_patches=n * pv.shape[0] + 64, max_prefill_tokens=n * L + 64)
    eng.load_state_dict(random_state_dict(cfg, seed=0, threads=16))
    pv_n, grid_n, ids_n = np.concatenate([pv] * n), np.concatenate([grid] * n), np.concatenate([ids] * n)
    slots = list(range(n))

    def run(forked):
        eng.set_sampling(0.0, 1.0, 0)
        eng.slots_reset()
        eng.set_eos([])
        for i in slots:
            eng.set_row_sampling(i, SamplingParams(temperature=1.0, top_p=0.95, seed=a.seed + i))
        eng.synchronize()
        t0 = time.perf_counter()
        if forked:
            eng.vit_forward(pv, grid)
            eng.slots_prefill(slots[:1], ids, [L], [new])
            eng.slots_fork(0, slots[1:])
        else:
            eng.vit_forward(pv_n, grid_n)
            eng.slots_prefill(slots, ids_n, [L] * n, [new] * n)
        eng.synchronize()
        t1 = time.perf_counter()
        done = 1
        while done < new:
            eng.slots_decode(a.chunk)
            done += a.chunk
        fin, lens = eng.slots_poll()                       # synchronises
        t2 = time.perf_counter()
        assert all(fin[s] == 1 and lens[s] == new for s in slots), (fin, lens)
        return (t1 - t0) * 1e3, (t2 - t0) * 1e3, [eng.slot_read(s, new).tolist() for s in slots]

    legs = ["independent"] if a.independent else ["forked", "independent"]
    tokens = {leg: run(leg == "forked")[2] for leg in legs}                 # the untimed round: code objects, graphs, allocations
    times = {leg: [] for leg in legs}
    for _ in range(a.reps):
        for leg in legs:                                   # alternating: both legs see the same neighbours on the machine
            first, total, toks = run(leg == "forked")
            assert toks == tokens[leg]
            times[leg].append((first, total))
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None
    except OSError:
        commit = None
    for leg in legs:
        f, t = [x[0] for x in times[leg]], [x[1] for x in times[leg]]
        print(json.dumps({"leg": leg, "n": n, "prompt_tokens": L, "patches": int(pv.shape[0]), "new_tokens": new, "reps": a.reps, "commit": commit,
                          "first_ms": {"median": round(statistics.median(f), 2), "min": round(min(f), 2), "max": round(max(f), 2)},
                          "total_ms": {"median": round(statistics.median(t), 2), "min": round(min(t), 2), "max": round(max(t), 2)}}), flush=True)
    if len(legs) == 2:
        print(json.dumps({"tokens_equal": tokens["forked"] == tokens["independent"],
                          "distinct_sequences": len({tuple(t) for t in tokens["forked"]})}), flush=True)


if __name__ == "__main__":
    main()
