#!/usr/bin/env python3
"""Suspend / resume against the two alternatives (profiles/kv_swap.txt).

    python tools/swap_bench.py [--dpi 200|300] [--reps 7] [--new-tokens 64] [--kv-cache-dtype bf16|fp8] [--tiny]

Workload: one synthetic A4 page through the processor (its real prompt: about 5k tokens at 200 dpi, the bench's page, about 11k at
300 dpi), full-size model with seeded random weights, one sequence.  Three legs, alternating, `reps` repetitions after one untimed
round of each, host clock around work that ends in a stream synchronise:

  swap        Engine.slot_suspend, then Engine.slot_resume of the row: the gather / scatter kernels through the 32-page staging buffer, one
              hipMemcpyAsync per chunk and direction.  Reported per direction, with the achieved host-link rate (bytes moved / time).
  per_page    the same bytes moved by one hipMemcpyAsync per (layer, page) between a device buffer laid out like the pool and pinned host
              memory, out and back, on one stream: what the swap would cost without the kernels.
  resubmit    the vision tower and the prefill of the same page: what a truncated request pays again when it is resubmitted.  Nothing of
              this leg is changed by the feature, so it is also the parent commit's figure.

Before the timed rounds the tool checks that a suspension leaves no trace: the K and V of the first and last layer around the start, a
page boundary and the end of the context are equal bit for bit before the suspension and after the resume, and the tokens of the following
chunk equal those of an undisturbed run.  One JSON line per leg, then the two ratios the design rests on.
"""
import argparse
import ctypes as C
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
    ap.add_argument("--reps", type=int, default=7)
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
    from dots_ocr_amd.synthetic import A4_200DPI, synth_page
    from dots_ocr_amd.weights import random_state_dict
    assert torch.cuda.is_available(), "swap_bench needs a GPU"
    cfg = DotsConfig.tiny(layers=2, v_layers=2) if a.tiny else DotsConfig()
    page = synth_page(0, (224, 168) if a.tiny else A4_200DPI if a.dpi == 200 else (2480, 3508))
    proc = DotsOcrProcessor(cfg)
    messages = [{"role": "user", "content": [{"type": "image", "image": page}, {"type": "text", "text": "Extract the text content from this image."}]}]
    text = proc.apply_chat_template(messages, tokenize=False, add_generation_prompt=True)
    inputs = proc(text=[text], images=[page], padding=True, return_tensors="pt")
    ids = inputs["input_ids"][0].numpy().astype(np.int32)
    pv = np.ascontiguousarray(inputs["pixel_values"].numpy(), dtype=np.float32)
    grid = inputs["image_grid_thw"].numpy().astype(np.int64)
    L, new = len(ids), a.new_tokens
    eng = Engine(cfg, max_batch=2, max_seq_len=L + new + 64, max_patches=pv.shape[0] + 64, max_prefill_tokens=L + 64, kv_cache_dtype=a.kv_cache_dtype)
    eng.load_state_dict(random_state_dict(cfg, seed=0, threads=16))
    layers, hkv = cfg.num_hidden_layers, cfg.num_key_value_heads
    page_bytes = hkv * 2 * 8192 * (1 if a.kv_cache_dtype == "fp8" else 2)              # one page of one layer

    def admit():
        eng.set_sampling(0.0, 1.0, 0)
        eng.slots_reset()
        eng.set_eos([])
        eng.synchronize()
        t0 = time.perf_counter()
        eng.vit_forward(pv, grid)
        eng.slots_prefill([0], ids, [L], [new])
        eng.synchronize()
        return (time.perf_counter() - t0) * 1e3

    # ---- a suspension leaves no trace
    admit()
    eng.slots_decode(a.chunk)
    _, lens = eng.slots_poll()
    want = eng.slot_read(0, int(lens[0])).tolist()
    eng.slots_decode(a.chunk)
    _, lens = eng.slots_poll()
    want2 = eng.slot_read(0, int(lens[0])).tolist()
    admit()
    eng.slots_decode(a.chunk)
    ctx = L + a.chunk
    n_pages = (ctx + 63) // 64
    eng.kv_swap_reserve((L + 2 * a.chunk + 63) // 64)      # what the timed rounds park, one chunk further on
    spots = sorted({0, 64 * (n_pages // 2) - 32, ctx - 64})

    def probe():
        return [eng.read_kv(layer, 0, p, 64, w) for layer in (0, layers - 1) for p in spots for w in ("k", "v")]

    before = probe()
    eng.slot_suspend(0)
    assert eng.kv_swap_info()[0] - eng.kv_swap_info()[1] == n_pages and eng.kv_pool_info()[0] == eng.kv_pool_info()[1]
    eng.slot_resume(0)
    kv_equal = all(np.array_equal(x, y) for x, y in zip(before, probe())) and all(x.any() for x in before)
    assert eng.slot_read(0, len(want)).tolist() == want
    eng.slots_decode(a.chunk)
    _, lens = eng.slots_poll()
    tokens_equal = eng.slot_read(0, int(lens[0])).tolist() == want2
    assert kv_equal and tokens_equal, (kv_equal, tokens_equal)
    ctx = L + 2 * a.chunk                                  # the row as the timed rounds find it
    n_pages = (ctx + 63) // 64

    # ---- the per-page leg's buffers: a device buffer laid out like the pool, pinned host memory laid out like the host space
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipMemcpyAsync.restype = C.c_int
    dev = torch.empty((layers, n_pages + 1, page_bytes), dtype=torch.uint8, device="cuda").random_(0, 256)
    host = torch.empty((n_pages, layers, page_bytes), dtype=torch.uint8).pin_memory()
    stream = torch.cuda.Stream()
    order = np.random.default_rng(0).permutation(n_pages)                              # scattered pages, as a pool's free list hands them out

    def per_page(to_host):
        stream.synchronize()
        t0 = time.perf_counter()
        for j in range(n_pages):
            for layer in range(layers):
                d, h = dev[layer, int(order[j])].data_ptr(), host[j, layer].data_ptr()
                rc = hip.hipMemcpyAsync(h, d, page_bytes, 2, stream.cuda_stream) if to_host else hip.hipMemcpyAsync(d, h, page_bytes, 1, stream.cuda_stream)
                assert rc == 0, rc
        stream.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def swap():
        eng.synchronize()
        t0 = time.perf_counter()
        eng.slot_suspend(0)                                # synchronises
        t1 = time.perf_counter()
        eng.slot_resume(0)                                 # synchronises
        return (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3

    swap(), per_page(True), per_page(False)                # the untimed round (admit() has run three times)
    t = {k: [] for k in ("suspend", "resume", "out", "back", "resubmit")}
    for _ in range(a.reps):                                # alternating: every leg sees the same neighbours on the machine
        s, r = swap()
        t["suspend"].append(s), t["resume"].append(r)
        t["out"].append(per_page(True)), t["back"].append(per_page(False))
    for _ in range(a.reps):
        t["resubmit"].append(admit())
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None
    except OSError:
        commit = None
    nbytes = n_pages * layers * page_bytes
    gbs = lambda ms: round(nbytes / (ms * 1e-3) / 1e9, 2)
    base = {"dpi": a.dpi, "prompt_tokens": L, "context": ctx, "pages": n_pages, "layers": layers, "page_bytes": page_bytes, "bytes": nbytes,
            "kv_cache_dtype": a.kv_cache_dtype, "reps": a.reps, "commit": commit}
    med = {k: statistics.median(v) for k, v in t.items()}
    print(json.dumps({"leg": "swap", **base, "suspend_ms": _stat(t["suspend"]), "resume_ms": _stat(t["resume"]),
                      "suspend_GBps": gbs(med["suspend"]), "resume_GBps": gbs(med["resume"]),
                      "kv_equal": kv_equal, "tokens_equal": tokens_equal}), flush=True)
    print(json.dumps({"leg": "per_page", **base, "copies_each_way": n_pages * layers, "out_ms": _stat(t["out"]), "back_ms": _stat(t["back"]),
                      "out_GBps": gbs(med["out"]), "back_GBps": gbs(med["back"])}), flush=True)
    print(json.dumps({"leg": "resubmit", **base, "patches": int(pv.shape[0]), "tower_prefill_ms": _stat(t["resubmit"])}), flush=True)
    both = med["suspend"] + med["resume"]
    print(json.dumps({"swap_ms": round(both, 3), "per_page_ms": round(med["out"] + med["back"], 3), "resubmit_ms": round(med["resubmit"], 3),
                      "per_page_over_swap": round((med["out"] + med["back"]) / both, 2), "resubmit_over_swap": round(med["resubmit"] / both, 2)}), flush=True)


if __name__ == "__main__":
    main()
