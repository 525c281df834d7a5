"""Prefix caching on one MI355X: what a hit saves.

Full-size random-weight model, the bench's A4 page, chunked prefill with passes of `--chunk` positions.

  ttft        time to the first token of one request through the engine's own calls (stream drained at both ends; median of --repeat):
              cold (tower + begin + every pass), a hit with the same image and another prompt (lookup + begin + passes behind the image's
              pages, no tower), and an exact repeat (the cap leaves the last page to fill).
  tail pass   the passes of such a hit alone — slots_prefill_advance until the slot runs, lookup and begin not counted.
  closed set  --pages pages, each read by one layout request and then — submitted when that one has finished, as a client that grounds the
              boxes of a layout does — by four grounding requests (the same image, other prompts), through ContinuousBatcher with the cache
              off and on: seconds, requests/s, tower calls; the tokens must be equal.

No test depends on these figures.

    python tools/prefix_cache_bench.py --pages 4
"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


class Counting:
    """forwards to the engine and counts the tower calls"""

    def __init__(self, engine):
        self._e, self.towers = engine, 0

    def __getattr__(self, name):
        attr = getattr(self._e, name)
        if name not in ("vit_forward", "vit_prefetch"):
            return attr

        def call(*a, **kw):
            self.towers += 1
            return attr(*a, **kw)
        return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=8)
    ap.add_argument("--chunk", type=int, default=2048, help="prompt positions per pass")
    ap.add_argument("--decode-chunk", type=int, default=16)
    ap.add_argument("--pages", type=int, default=4)
    ap.add_argument("--tokens", type=int, default=64, help="tokens generated per request of the closed set")
    ap.add_argument("--repeat", type=int, default=5)
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
    sd = random_state_dict(cfg, seed=a.seed, threads=min(16, os.cpu_count() or 8))
    dev = torch.device("cuda", 0)
    pages = []
    for i in range(a.pages):
        feat, g = preprocess_image(synth_page(i, size))
        pages.append(dict(pv=torch.from_numpy(feat).to(dev), grid=np.asarray([g], np.int64), pads=int(g[1] * g[2] // 4),
                          key=hashlib.blake2b(feat.tobytes(), digest_size=16).digest()))

    def prompt(page, k):
        """the page's chat head and pads, then the k-th prompt text"""
        ids = synth_prompt_ids(cfg, pages[page]["pads"], seed=1000 * page)
        tail = len(ids) - 3 - pages[page]["pads"]
        ids[len(ids) - tail:] = np.random.default_rng(7 + 1000 * page + k).integers(0, min(cfg.vocab_size, cfg.image_token_id) - 1, tail)
        return ids

    plen = len(prompt(0, 0))
    chunk = min(a.chunk, (plen + 63) // 64 * 64)
    eng = Engine(cfg, device=0, max_batch=a.slots, max_seq_len=plen + a.tokens + 64, max_patches=a.slots * pages[0]["pv"].shape[0] + 64,
                 max_prefill_tokens=max(chunk, plen + 64))
    eng.load_state_dict(sd)
    eng.set_sampling(0.0, 1.0, 0)
    eng.set_eos([])
    res = {"workload": a.workload, "prompt_tokens": plen, "image_tokens": pages[0]["pads"], "pass_positions": chunk}

    # ---- one request through the engine's own calls
    def one(ids, page, what):
        """-> (ms to the first token, ms of the passes alone, hit tokens)"""
        eng.synchronize()
        t0 = time.perf_counter()
        lease, hit, tower = eng.prefix_cache_lookup(ids, pages[page]["key"])
        assert (hit > 0) == (what != "cold") and tower == (what == "cold"), (what, hit, tower)
        if tower:
            eng.vit_forward(pages[page]["pv"].data_ptr(), pages[page]["grid"], on_device=True)
        eng.slots_prefill_begin_cached([1], ids, [len(ids)], [4], [lease], [pages[page]["key"]])
        eng.synchronize()
        t1 = time.perf_counter()
        while eng.slots_prefill_advance(chunk) > 0:
            pass
        eng.synchronize()
        t2 = time.perf_counter()
        eng.slot_release(1)
        return 1e3 * (t2 - t0), 1e3 * (t2 - t1), hit

    runs = {"cold": [], "hit_other_prompt": [], "exact_repeat": []}
    for r in range(a.repeat + 1):                     # the first round warms buffers and is dropped
        eng.slots_reset()
        eng.prefix_cache_enable(False)
        eng.prefix_cache_enable(True)
        got = {"cold": one(prompt(0, 0), 0, "cold"), "hit_other_prompt": one(prompt(0, 1), 0, "hit"), "exact_repeat": one(prompt(0, 0), 0, "hit")}
        if r:
            for k, v in got.items():
                runs[k].append(v)
    for k, v in runs.items():
        res[f"ttft[{k}]"] = {"ms": round(float(np.median([x[0] for x in v])), 2), "passes_alone_ms": round(float(np.median([x[1] for x in v])), 2),
                             "hit_tokens": v[0][2], "filled_tokens": plen - v[0][2]}
    eng.slots_reset()
    eng.prefix_cache_enable(False)

    # ---- closed set: every page under one layout prompt and four grounding prompts
    def serve(on):
        ce = Counting(eng)
        cb = ContinuousBatcher(ce, chunk=a.decode_chunk, prefill_chunk=chunk, prefix_caching=on)

        def req(p, k):
            return Request(prompt(p, k), pages[p]["pv"], pages[p]["grid"], a.tokens, image_key=pages[p]["key"], tag=(p, k))
        eng.synchronize()
        t0 = time.perf_counter()
        for p in range(a.pages):
            cb.submit(req(p, 0))
        outs = {}
        while not cb.idle:
            for _, r, toks in cb.step():
                outs[r.tag] = toks
                if r.tag[1] == 0:                     # the layout is there: its four grounding requests follow
                    for k in range(1, 5):
                        cb.submit(req(r.tag[0], k))
        eng.synchronize()
        dt = time.perf_counter() - t0
        out = {"seconds": round(dt, 3), "requests_per_s": round(len(outs) / dt, 3), "tower_calls": ce.towers, "fill_passes": cb.fill_passes,
               "prefix_hits": cb.prefix_hits, "prefix_hit_tokens": cb.prefix_hit_tokens}
        if on:
            out["cache"] = eng.prefix_cache_info()
            eng.slots_reset()
            eng.prefix_cache_enable(False)
        return outs, out

    outs = {}
    for on in (False, True, False, True):             # twice, alternating: the second round is the one reported
        outs[on], res[f"closed_set[{'on' if on else 'off'}]"] = serve(on)
    res["closed_set_tokens_identical"] = bool(sorted(outs[False]) == sorted(outs[True]) and all(np.array_equal(outs[False][t], outs[True][t]) for t in outs[False]))
    eng.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
