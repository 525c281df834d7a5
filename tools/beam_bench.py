#!/usr/bin/env python3
"""A beam group against independent greedy rows of the same page (profiles/beam_search.txt).

    python tools/beam_bench.py [--reps 5] [--beams 4] [--new-tokens 256]
        both legs, alternating, in one process: `beam` (one tower, one prefill, Engine.slots_beam, B rows whose selection and page
        reorder run inside the captured steps) and `independent` (the page's pixels and prompt B times in one group: B towers, B
        prefills, B plain greedy rows), after one untimed round of each
    python tools/beam_bench.py --independent
        the independent leg alone.  It uses only calls that exist without slots_beam, so it also runs on the commit before the feature:
        that run is the baseline

Workload: one synthetic A4 page at 200 dpi through the processor (its real prompt), full-size model with seeded random weights, B = 4,
256 steps, no EOS.  Per repetition, host clock from before the tower is enqueued to a stream synchronise: `first_ms` = until the first
step's tokens exist (the group's first selection / the B first tokens), `step_ms` = the decode chunks' time per step.  One JSON line per
leg with the median and the spread (min, max) over the repetitions.  With both legs, a last line gives `beam_step_extra_ms` = the
difference of the legs' step_ms medians — what beam_select (with its logprob partials) and beam_reorder (whose tail copy moves up to
B x layers x page bytes per step) add to a step of B rows, the decode kernels being the same launches over the same rows in both legs —
and its share of the beam leg's step, next to the bytes the tail copies may move per step at most.
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
    ap.add_argument("--beams", type=int, default=4)
    ap.add_argument("--new-tokens", type=int, default=256)
    ap.add_argument("--chunk", type=int, default=16)
    ap.add_argument("--independent", action="store_true", help="the independent leg only (runs without slots_beam)")
    ap.add_argument("--tiny", action="store_true", help="tiny dimensions and a small page: a rehearsal of the plumbing, not a measurement")
    a = ap.parse_args()
    import torch
    from dots_ocr_amd.config import DotsConfig
    from dots_ocr_amd.engine import Engine
    from dots_ocr_amd.processing import DotsOcrProcessor
    from dots_ocr_amd.synthetic import A4_200DPI, synth_page
    from dots_ocr_amd.weights import random_state_dict
    assert torch.cuda.is_available(), "beam_bench needs a GPU"
    cfg = DotsConfig.tiny(layers=2, v_layers=2) if a.tiny else DotsConfig()
    page = synth_page(0, (224, 168) if a.tiny else A4_200DPI)
    proc = DotsOcrProcessor(cfg)
    messages = [{"role": "user", "content": [{"type": "image", "image": page}, {"type": "text", "text": "Extract the text content from this image."}]}]
    text = proc.apply_chat_template(messages, tokenize=False, add_generation_prompt=True)
    inputs = proc(text=[text], images=[page], padding=True, return_tensors="pt")
    ids = inputs["input_ids"][0].numpy().astype(np.int32)
    pv = np.ascontiguousarray(inputs["pixel_values"].numpy(), dtype=np.float32)
    grid = inputs["image_grid_thw"].numpy().astype(np.int64)
    n, L, new = a.beams, len(ids), a.new_tokens
    eng = Engine(cfg, max_batch=n, max_seq_len=L + new + 64, max_patches=n * pv.shape[0] + 64, max_prefill_tokens=n * L + 64)
    eng.load_state_dict(random_state_dict(cfg, seed=0, threads=16))
    pv_n, grid_n, ids_n = np.concatenate([pv] * n), np.concatenate([grid] * n), np.concatenate([ids] * n)
    slots = list(range(n))
    steps = -(-(new - 1) // a.chunk) * a.chunk              # decode steps issued: whole chunks

    def run(beam):
        eng.set_sampling(0.0, 1.0, 0)
        eng.slots_reset()
        eng.set_eos([])
        eng.synchronize()
        t0 = time.perf_counter()
        if beam:
            eng.vit_forward(pv, grid)
            eng.slots_prefill(slots[:1], ids, [L], [new])
            eng.slots_beam(0, slots[1:])
        else:
            eng.vit_forward(pv_n, grid_n)
            eng.slots_prefill(slots, ids_n, [L] * n, [new] * n)
        eng.synchronize()
        t1 = time.perf_counter()
        for _ in range(steps // a.chunk):
            eng.slots_decode(a.chunk)
        fin, lens = eng.slots_poll()                       # synchronises
        t2 = time.perf_counter()
        assert all(fin[s] == 1 and lens[s] == new for s in slots), (fin, lens)
        if beam:
            tr = eng.beam_read(0)
            out = (tr["tokens"].tolist(), tr["parents"].tolist(), tr["cum"].view(np.uint32).tolist())
            live = [tr["parents"][:, t][tr["parents"][:, t] >= 0] for t in range(1, tr["steps"])]
            forks = int(sum((np.bincount(p, minlength=n) >= 2).any() for p in live))
        else:
            out, forks = [eng.slot_read(s, new).tolist() for s in slots], 0
        return (t1 - t0) * 1e3, (t2 - t1) * 1e3 / steps, out, forks

    legs = ["independent"] if a.independent else ["beam", "independent"]
    first = {leg: run(leg == "beam") for leg in legs}                       # the untimed round: code objects, graphs, allocations
    times = {leg: [] for leg in legs}
    for _ in range(a.reps):
        for leg in legs:                                   # alternating: both legs see the same neighbours on the machine
            f, s, out, _ = run(leg == "beam")
            assert out == first[leg][2]
            times[leg].append((f, s))
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None
    except OSError:
        commit = None
    med = {}
    for leg in legs:
        f, s = [x[0] for x in times[leg]], [x[1] for x in times[leg]]
        med[leg] = statistics.median(s)
        print(json.dumps({"leg": leg, "beams": n, "prompt_tokens": L, "patches": int(pv.shape[0]), "new_tokens": new, "decode_steps": steps,
                          "reps": a.reps, "commit": commit,
                          "first_ms": {"median": round(statistics.median(f), 2), "min": round(min(f), 2), "max": round(max(f), 2)},
                          "step_ms": {"median": round(med[leg], 4), "min": round(min(s), 4), "max": round(max(s), 4)},
                          **({"steps_with_a_fork": first[leg][3]} if leg == "beam" else {})}), flush=True)
    if len(legs) == 2:
        page_bytes = cfg.num_key_value_heads * 2 * 8192 * (1 if eng.kv_cache_dtype == "fp8" else 2)
        extra = med["beam"] - med["independent"]
        print(json.dumps({"beam_step_extra_ms": round(extra, 4), "share_of_beam_step": round(extra / med["beam"], 4),
                          "tail_copy_bytes_per_step_max": n * cfg.num_hidden_layers * page_bytes}), flush=True)


if __name__ == "__main__":
    main()
