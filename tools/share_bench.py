#!/usr/bin/env python3
"""Shared-prefix decode attention against the per-row kernel on forked rows (profiles/shared_prefix_attention.txt).

    python tools/share_bench.py [--reps 5] [--steps 128] [--legs fork8,fork64,indep8]
        per leg, in one process, the switch off and on alternating after one untimed round of each:
          fork8    8 slots: one A4 page prefilled once and forked into n = 8 sampled rows
          fork64   64 slots: 8 prefills of the page, each forked into 8
          indep8   8 slots: the page prefilled 8 times — nobody shares, the switch costs its dirty-flag check
    python tools/share_bench.py --baseline [--legs ...]
        the switch-off side alone.  It uses only calls that exist without the feature, so it also runs on the commit before it: that
        run is the yardstick for "no cost when unused"

Workload: one synthetic A4 page at 200 dpi through the processor (its real prompt), full-size model with seeded random weights, sampled
rows (temperature 1.0, top_p 0.95, one seed per row), no EOS.  Timed per repetition: `--steps` decode steps in chunks of 16, host clock from
a stream synchronise before the first chunk to one behind the last (prefill, tower and fork are outside the window).  One JSON line per
(leg, switch) with the median and the spread of the time per step, the plan's counters, and whether both sides gave the same tokens (they
must).  The time of the attention launches alone is the kernel trace's: run the tool under `rocprofv3 --kernel-trace --stats` with
--reps 1 and read the decode_attn_* rows.
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

LEGS = {"fork8": (1, 8), "fork64": (8, 8), "indep8": (8, 1)}      # leg -> (prefills, rows per prefill)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--chunk", type=int, default=16)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--legs", default="fork8,fork64,indep8")
    ap.add_argument("--baseline", action="store_true", help="the switch-off side only (runs without the feature)")
    ap.add_argument("--tiny", action="store_true", help="tiny dimensions and a small page: a rehearsal of the plumbing, not a measurement")
    a = ap.parse_args()
    import torch
    from dots_ocr_amd.config import DotsConfig
    from dots_ocr_amd.engine import Engine, SamplingParams
    from dots_ocr_amd.processing import DotsOcrProcessor
    from dots_ocr_amd.synthetic import A4_200DPI, synth_page
    from dots_ocr_amd.weights import random_state_dict
    assert torch.cuda.is_available(), "share_bench needs a GPU"
    legs = [leg for leg in a.legs.split(",") if leg]
    assert legs and all(leg in LEGS for leg in legs), f"legs are {sorted(LEGS)}"
    cfg = DotsConfig.tiny(layers=2, v_layers=2) if a.tiny else DotsConfig()
    page = synth_page(0, (448, 336) if a.tiny else A4_200DPI)
    proc = DotsOcrProcessor(cfg)
    messages = [{"role": "user", "content": [{"type": "image", "image": page}, {"type": "text", "text": "Extract the text content from this image."}]}]
    text = proc.apply_chat_template(messages, tokenize=False, add_generation_prompt=True)
    inputs = proc(text=[text], images=[page], padding=True, return_tensors="pt")
    ids = inputs["input_ids"][0].numpy().astype(np.int32)
    pv = np.ascontiguousarray(inputs["pixel_values"].numpy(), dtype=np.float32)
    grid = inputs["image_grid_thw"].numpy().astype(np.int64)
    L, new = len(ids), a.steps + 1
    rows_max = max(LEGS[leg][0] * LEGS[leg][1] for leg in legs)
    eng = Engine(cfg, max_batch=rows_max, max_seq_len=L + new + 64, max_patches=pv.shape[0] + 64, max_prefill_tokens=L + 64)
    eng.load_state_dict(random_state_dict(cfg, seed=0, threads=16))
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None
    except OSError:
        commit = None

    def run(leg, on):
        prefills, per = LEGS[leg]
        slots = list(range(prefills * per))
        eng.set_sampling(0.0, 1.0, 0)
        eng.slots_reset()
        eng.set_eos([])
        if not a.baseline:
            eng.set_shared_prefix_attention(on)
        for i in slots:
            eng.set_row_sampling(i, SamplingParams(temperature=1.0, top_p=0.95, seed=a.seed + i))
        for p in range(prefills):
            eng.vit_forward(pv, grid)
            eng.slots_prefill([p * per], ids, [L], [new])
            if per > 1:
                eng.slots_fork(p * per, slots[p * per + 1:(p + 1) * per])
        eng.synchronize()
        t0 = time.perf_counter()
        for _ in range(0, a.steps, a.chunk):
            eng.slots_decode(a.chunk)
        eng.synchronize()
        t1 = time.perf_counter()
        info = None if a.baseline else eng.shared_prefix_info()
        toks = [eng.slot_read(s, new).tolist() for s in slots]
        if not a.baseline:
            eng.set_shared_prefix_attention(False)
        return (t1 - t0) * 1e3 / a.steps, info, toks

    sides = [False] if a.baseline else [False, True]
    for leg in legs:
        tokens = {on: run(leg, on)[2] for on in sides}                    # the untimed round: code objects, graphs, allocations
        times, infos = {on: [] for on in sides}, {}
        for _ in range(a.reps):
            for on in sides:                                              # alternating: both sides see the same neighbours on the machine
                ms, info, toks = run(leg, on)
                assert toks == tokens[on]
                times[on].append(ms)
                infos[on] = info
        for on in sides:
            t = times[on]
            line = {"leg": leg, "shared_prefix_attention": None if a.baseline else on, "rows": LEGS[leg][0] * LEGS[leg][1], "prompt_tokens": L,
                    "steps": a.steps, "reps": a.reps, "commit": commit,
                    "step_ms": {"median": round(statistics.median(t), 4), "min": round(min(t), 4), "max": round(max(t), 4)}}
            if infos[on] is not None:
                line["plan"] = {k: infos[on][k] for k in ("items", "rows", "pairs")}
            print(json.dumps(line), flush=True)
        if len(sides) == 2:
            off, on_ = statistics.median(times[False]), statistics.median(times[True])
            print(json.dumps({"leg": leg, "tokens_equal": tokens[False] == tokens[True], "step_ms_on_over_off": round(on_ / off, 4)}), flush=True)


if __name__ == "__main__":
    main()
