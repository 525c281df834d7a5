#!/usr/bin/env python3
"""Several prompts over one page: the fan-out against independent requests (profiles/slot_extend.txt).

    python tools/extend_bench.py [--m 2 4 8] [--dpi 200|300] [--reps 5] [--new-tokens 64] [--kv-cache-dtype bf16|fp8] [--tiny]

Workload: one synthetic A4 page through the processor, full-size model with seeded random weights, m grounding prompts (the reference's
prompt_grounding_ocr text, each with its own bounding box) read off that page, `new_tokens` greedy tokens each, no EOS.  Two legs through
the scheduler on the same engine with m slots, alternating, `reps` repetitions after one untimed round of each, host clock around
ContinuousBatcher.run (which ends in a poll):

  independent  m requests, each with the whole prompt and the page's pixels: m towers and m prefills in one admission.  Nothing of this
               leg is changed by the feature, so it is also the parent commit's figure.
  fan_out      one Request(suffixes=...): one tower, one prefill of the common prefix, one fork, one Engine.slots_extend.

Then the extend alone on a prefilled and forked prefix: its wall time and, from it, the time per chunk of at most max_batch rows.  The
decode steps are the same in both legs, so the difference of the walls is what admission costs.  One JSON line per m.
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
    ap.add_argument("--m", type=int, nargs="+", default=[2, 4, 8])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--new-tokens", type=int, default=64)
    ap.add_argument("--chunk", type=int, default=16)
    ap.add_argument("--dpi", type=int, choices=[200, 300], default=200, help="the A4 page's resolution: 1654 x 2339 or 2480 x 3508 pixels")
    ap.add_argument("--kv-cache-dtype", choices=["bf16", "fp8"], default="bf16")
    ap.add_argument("--tiny", action="store_true", help="tiny dimensions and a small page: a rehearsal of the plumbing, not a measurement")
    a = ap.parse_args()
    import torch
    from dots_ocr_amd.config import DotsConfig
    from dots_ocr_amd.engine import Engine
    from dots_ocr_amd.processing import DotsOcrProcessor
    from dots_ocr_amd.prompts import dict_promptmode_to_prompt
    from dots_ocr_amd.scheduler import ContinuousBatcher, Request, split_common_prefix
    from dots_ocr_amd.synthetic import A4_200DPI, synth_page
    from dots_ocr_amd.weights import random_state_dict
    assert torch.cuda.is_available(), "extend_bench needs a GPU"
    cfg = DotsConfig.tiny(layers=2, v_layers=2) if a.tiny else DotsConfig()
    page = synth_page(0, (224, 168) if a.tiny else A4_200DPI if a.dpi == 200 else (2480, 3508))
    proc = DotsOcrProcessor(cfg)
    m_max, new = max(a.m), a.new_tokens
    rng = np.random.default_rng(0)
    prompts = []
    for _ in range(m_max):
        x1, y1 = int(rng.integers(0, page.width // 2)), int(rng.integers(0, page.height // 2))
        prompts.append(dict_promptmode_to_prompt["prompt_grounding_ocr"] + str([x1, y1, x1 + int(rng.integers(50, page.width // 2)),
                                                                                 y1 + int(rng.integers(20, page.height // 2))]))

    def text_of(p):
        messages = [{"role": "user", "content": [{"type": "image", "image": page}, {"type": "text", "text": p}]}]
        return proc.apply_chat_template(messages, tokenize=False, add_generation_prompt=True)
    inputs = proc(text=[text_of(prompts[0])], images=[page], padding=True, return_tensors="pt")
    pv = np.ascontiguousarray(inputs["pixel_values"].numpy(), dtype=np.float32)
    grid = inputs["image_grid_thw"].numpy().astype(np.int64)
    seqs = [inputs["input_ids"][0].tolist()] + [proc.encode_prompt(text_of(p), grid.tolist()) for p in prompts[1:]]
    L = max(len(s) for s in seqs)
    eng = Engine(cfg, max_batch=m_max, max_seq_len=L + new + 64, max_patches=m_max * pv.shape[0] + 64, max_prefill_tokens=m_max * L + 64,
                 kv_cache_dtype=a.kv_cache_dtype)
    eng.load_state_dict(random_state_dict(cfg, seed=0, threads=16))
    eng.set_sampling(0.0, 1.0, 0)
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None
    except OSError:
        commit = None

    for m in a.m:
        prefix, sufs = split_common_prefix(seqs[:m])
        assert cfg.image_token_id not in [t for s in sufs for t in s]

        def independent():
            reqs = [Request(np.asarray(s, np.int32), pv, grid, new) for s in seqs[:m]]
            cb = ContinuousBatcher(eng, eos_ids=(), chunk=a.chunk)
            eng.synchronize()
            t0 = time.perf_counter()
            outs = cb.run(reqs)
            return (time.perf_counter() - t0) * 1e3, [o.tolist() for o in outs], cb.admissions

        def fan_out():
            r = Request(np.asarray(prefix, np.int32), pv, grid, new, suffixes=sufs)
            cb = ContinuousBatcher(eng, eos_ids=(), chunk=a.chunk)
            eng.synchronize()
            t0 = time.perf_counter()
            cb.run([r])
            return (time.perf_counter() - t0) * 1e3, [o.tolist() for o in r.outputs], cb.admissions

        def extend_alone():
            eng.slots_reset()
            eng.set_eos([])
            eng.vit_forward(pv, grid)
            eng.slots_prefill([0], np.asarray(prefix, np.int32), [len(prefix)], [new])
            eng.slots_fork(0, list(range(1, m)))
            eng.synchronize()
            t0 = time.perf_counter()
            eng.slots_extend(list(range(m)), sufs, max_new_tokens=new)      # synchronises
            ms = (time.perf_counter() - t0) * 1e3
            eng.slots_reset()
            return ms

        _, toks_i, adm = independent()                     # the untimed round
        _, toks_f, _ = fan_out()
        extend_alone()
        # both are valid evaluations of the same sequences: the prefill kernels on one side, the decode kernels on the other
        agree = sum(x == y for ti, tf in zip(toks_i, toks_f) for x, y in zip(ti, tf)) / float(m * new)
        t = {"independent": [], "fan_out": [], "extend": []}
        for _ in range(a.reps):                            # alternating: every leg sees the same neighbours on the machine
            t["independent"].append(independent()[0])
            t["fan_out"].append(fan_out()[0])
            t["extend"].append(extend_alone())
        rows = sum(len(s) for s in sufs)
        chunks = -(-rows // m_max)
        med = {k: statistics.median(v) for k, v in t.items()}
        print(json.dumps({"m": m, "dpi": a.dpi, "prompt_tokens": L, "prefix_tokens": len(prefix), "suffix_tokens": [len(s) for s in sufs],
                          "patches": int(pv.shape[0]), "new_tokens": new, "slots": m_max, "kv_cache_dtype": a.kv_cache_dtype, "reps": a.reps,
                          "independent_admissions": adm, "independent_ms": _stat(t["independent"]), "fan_out_ms": _stat(t["fan_out"]),
                          "extend_ms": _stat(t["extend"]), "extend_rows": rows, "extend_chunks": chunks,
                          "extend_ms_per_chunk": round(med["extend"] / chunks, 3),
                          "independent_over_fan_out": round(med["independent"] / med["fan_out"], 2), "token_agreement": round(agree, 3),
                          "commit": commit}), flush=True)


if __name__ == "__main__":
    main()
