"""Chunked prefill on one MI355X: what filling a prompt in passes does to the rows that are already decoding.

Full-size random-weight model, the bench's A4 page, `--slots` slots.  For chunking off and for every N of --chunks:

  admission   slots - 1 rows are decoding; one more request is admitted.  Reported: the longest gap between two decode chunks of the
              running rows (end of one chunk to the start of the next, the stream drained at both), and the admitted request's time to
              its first token (submit to the step in which it joined the running rows).
  serve       pages/s of a short closed set (`--pages` pages, seeded length caps around `--mean-tokens`), continuous batching.
  kernel      the paged attention kernel alone (one A4 prompt, prefix 0, its pages in pool order) against flash_attn_kernel<CAUSAL> on the
              same shape: milliseconds per launch through the single-kernel entry points (host time around a synchronising call, best of 5).

No test depends on these figures.

    python tools/chunked_prefill_bench.py --slots 8 --chunks 1024,2048,4096
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


class Timed:
    """forwards to the engine; every decode chunk is bracketed by a drained stream and its (start, end) written down"""

    def __init__(self, engine):
        self._e, self.chunks = engine, []

    def __getattr__(self, name):
        attr = getattr(self._e, name)
        if name != "slots_decode":
            return attr

        def decode(n):
            self._e.synchronize()
            t0 = time.perf_counter()
            attr(n)
            self._e.synchronize()
            self.chunks.append((t0, time.perf_counter()))
        return decode


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=8)
    ap.add_argument("--chunks", default="1024,2048,4096")
    ap.add_argument("--chunk", type=int, default=16, help="decode steps per chunk")
    ap.add_argument("--pages", type=int, default=16)
    ap.add_argument("--mean-tokens", type=int, default=256)
    ap.add_argument("--workload", default="a4", choices=["a4", "tiny"])
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()

    from dots_ocr_amd.config import DotsConfig
    from dots_ocr_amd.engine import Engine
    from dots_ocr_amd.image_utils import preprocess_image
    from dots_ocr_amd.scheduler import ContinuousBatcher, Request
    from dots_ocr_amd.synthetic import A4_200DPI, synth_page, synth_prompt_ids
    from dots_ocr_amd.weights import random_state_dict

    if a.workload == "tiny":
        cfg, size = DotsConfig.tiny(layers=4, v_layers=4), (420, 588)
    else:
        cfg, size = DotsConfig(), A4_200DPI
    modes = [None] + [int(x) for x in a.chunks.split(",") if x]
    sd = random_state_dict(cfg, seed=a.seed, threads=min(16, os.cpu_count() or 8))
    distinct = min(a.pages, 4)
    feats, grids = zip(*(preprocess_image(synth_page(i, size)) for i in range(distinct)))
    dev = torch.device("cuda", 0)
    pv = [torch.from_numpy(f).to(dev) for f in feats]
    grid = [np.asarray([g], np.int64) for g in grids]
    n_req = max(a.pages, a.slots)
    prompts = [synth_prompt_ids(cfg, int(grids[i % distinct][1] * grids[i % distinct][2] // 4), seed=i) for i in range(n_req)]
    plen = max(len(p) for p in prompts)
    rng = np.random.default_rng(a.seed)
    caps = rng.integers(a.mean_tokens // 4, 7 * a.mean_tokens // 4 + 1, size=a.pages).astype(int).tolist()
    smallest = min(m for m in modes if m is not None)
    long_cap = (a.slots * -(-plen // smallest) + 40) * a.chunk      # the rows still decode when the last of them has been filled in passes
    eng = Engine(cfg, device=0, max_batch=a.slots, max_seq_len=plen + max(max(caps), long_cap) + 64, max_patches=a.slots * feats[0].shape[0] + 64,
                 max_prefill_tokens=a.slots * plen + 64)
    eng.load_state_dict(sd)
    eng.set_sampling(0.0, 1.0, 0)
    modes = [m for m in modes if m is None or m <= eng.max_prefill_tokens]
    res = {"workload": a.workload, "slots": a.slots, "prompt_tokens": plen, "decode_chunk": a.chunk}

    def req(i, cap):
        return Request(prompts[i], pv[i % distinct], grid[i % distinct], cap)

    def kw(m):
        return {} if m is None else {"prefill_chunk": m}

    # ---- admission: slots - 1 rows decode, one request is admitted
    def admission(m):
        te = Timed(eng)
        cb = ContinuousBatcher(te, chunk=a.chunk, headroom_pages=0, **kw(m))      # the pool holds every row at its cap: nothing waits for pages
        for i in range(a.slots - 1):
            cb.submit(req(i, long_cap))
        while len(cb.running) < a.slots - 1:
            cb.step()
        for _ in range(3):
            cb.step()
        first = len(te.chunks) - 1                   # the last chunk before the request arrives: the first gap starts at its end
        eng.synchronize()
        t_sub = time.perf_counter()
        rid = cb.submit(req(a.slots - 1, long_cap))
        t_first = None
        for _ in range(200):
            cb.step()
            if t_first is None and any(r == rid for r, _ in cb.running.values()):
                eng.synchronize()
                t_first = time.perf_counter()
            if t_first is not None and len(te.chunks) - first >= 6:
                break
        if t_first is None:
            raise RuntimeError(f"the request was never admitted (chunk {m}): running {sorted(cb.running)}, pending {len(cb.pending)}, filling "
                               f"{[x[0] for x in cb.filling]}, pool {eng.kv_pool_info()}, decode chunks {len(te.chunks) - first}, poll {eng.slots_poll()[0].tolist()}")
        chunks = te.chunks[first:]
        gaps = [b[0] - x[1] for x, b in zip(chunks, chunks[1:])]
        durs = [e1 - s for s, e1 in chunks]
        return {"longest_gap_ms": round(1e3 * max(gaps), 2), "median_gap_ms": round(1e3 * float(np.median(gaps)), 3),
                "median_decode_chunk_ms": round(1e3 * float(np.median(durs)), 2), "time_to_first_token_ms": round(1e3 * (t_first - t_sub), 2),
                "passes": cb.fill_passes}

    for m in modes + modes:                            # twice, interleaved: the second round is the one reported (graphs and buffers warm)
        res[f"admission[{m or 'off'}]"] = admission(m)

    # ---- serve: a short closed set
    def serve(m):
        cb = ContinuousBatcher(eng, chunk=a.chunk, **kw(m))
        eng.synchronize()
        t0 = time.perf_counter()
        outs = cb.run([req(i, caps[i]) for i in range(a.pages)])
        eng.synchronize()
        dt = time.perf_counter() - t0
        return outs, {"seconds": round(dt, 3), "pages_per_s": round(a.pages / dt, 3), "tokens_per_s": round(sum(caps) / dt, 1)}

    outs = {}
    for m in modes:
        outs[m], res[f"serve[{m or 'off'}]"] = serve(m)
    chunked = [m for m in modes if m is not None]
    res["serve_tokens_identical_across_chunks"] = bool(all(all(np.array_equal(x, y) for x, y in zip(outs[chunked[0]], outs[m])) for m in chunked[1:]))

    # ---- the kernel alone against the causal flash kernel, one prompt
    Hq, Hkv, T = cfg.num_attention_heads, cfg.num_key_value_heads, plen
    g = torch.Generator(device="cuda").manual_seed(1)
    q = torch.randn(Hq, T, 128, device="cuda", generator=g).bfloat16()
    k = torch.randn(Hkv * T + 64, 128, device="cuda", generator=g).bfloat16()
    pages = (T + 63) // 64
    vt = torch.randn(Hkv, 128, pages * 64, device="cuda", generator=g).bfloat16()
    pool = torch.randn(pages + 1, Hkv, 2, 8192, device="cuda", generator=g).bfloat16()
    table = torch.arange(pages, dtype=torch.int32, device="cuda").view(1, -1).contiguous()
    out = torch.zeros(T, Hq * 128, dtype=torch.bfloat16, device="cuda")
    cu = np.array([0, T], np.int32)
    scale = 1.0 / np.sqrt(128.0)
    torch.cuda.synchronize()

    def best(fn, n=5):
        ts = []
        for _ in range(n):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        return round(1e3 * min(ts), 3)
    res["kernel_ms"] = {
        "flash_attn_causal": best(lambda: eng.op_flash_attn(q.data_ptr(), k.data_ptr(), vt.data_ptr(), out.data_ptr(), cu, Hq, Hkv, True, scale)),
        "flash_attn_paged": best(lambda: eng.op_flash_attn_paged(q.data_ptr(), pool.data_ptr(), table.data_ptr(), pages, 1, out.data_ptr(), [0], [T], Hq,
                                                                   Hkv, scale)),
        "tokens": T, "note": "host time around one synchronising single-kernel call (work list upload included), best of 5"}
    eng.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
