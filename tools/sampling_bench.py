#!/usr/bin/env python3
"""The token-selection stage at the real vocabulary (V = 151 936; profiles/sampling_rows.txt).

    python tools/sampling_bench.py [--rows 1 8 64] [--iters 200]
        per row count, mean time of one stage (HIP events around `iters` replays after a warm-up, one process):
          argmax      the engine-wide greedy pair (argmax_partial_kernel + argmax_step_kernel)
          sampler     the engine-wide sampler, T = 0.7, top_p = 0.9 (sample_step_kernel)
          rows_greedy the per-row stage, every row greedy without penalties
          rows_loaded the per-row stage, every row at T = 0.1, top_p = 0.9, top_k = 50 + all three penalties
    python tools/sampling_bench.py --rules [--rows 1 8 64] [--iters 200]
        the logit-rule leg (profiles/logit_rules.txt): rows_greedy and rows_loaded as above, each again with every row
        carrying a 300-entry bias and a 5 000-id allowed list (+ min_tokens in force: two EOS ids and four stop ids masked), and the
        host-side cost of setting one row's rules (Engine.set_row_logit_rules, mean wall time over 50 calls, synchronised at the end)
    python tools/sampling_bench.py --guided [--rows 1 8 64] [--iters 200]
        the guided-decoding leg (profiles/guided.txt): rows_greedy and rows_loaded with 0 / 1 / all rows following the layout
        guide (guided.layout_schema) from assorted states over a synthetic byte-level token table, the mask kernel included; the ruled
        stage of the same build beside them; and the host-side cost of Engine.create_guide and Engine.set_row_guide
    python tools/sampling_bench.py --ngram [--rows 1 8 64] [--iters 200]
        the n-gram leg (profiles/ngram.txt): rows_greedy and rows_loaded with every row carrying a no-repeat rule n = 30, first
        with W = 90 and then with W = 0, the ban kernel included, over generated histories of 64 / 1024 / 16 384 tokens — random ids
        (ordinary text: a candidate is dropped at its first token) and a period-7 loop (the worst case: every candidate matches all 29) —
        beside the same stage of the same build without a rule; and the host-side cost of Engine.set_row_ngram
    python tools/sampling_bench.py --rows 64 --iters 20
        under `rocprofv3 --kernel-trace --stats -- python tools/sampling_bench.py ...` for the per-kernel split.
Logits: a seeded N(0, 2) background with 64 planted tokens in [8, 14] per row (an LM-like peaked head); histories of 1200 prompt ids
and 300 generated ids.  One JSON line per measurement on stdout.
"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np  # noqa: E402

V = 151936


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rules", action="store_true", help="the logit-rule leg instead of the four stages")
    ap.add_argument("--guided", action="store_true", help="the guided-decoding leg instead of the four stages")
    ap.add_argument("--ngram", action="store_true", help="the no-repeat n-gram leg instead of the four stages")
    a = ap.parse_args()
    if a.guided:
        return guided_leg(a)
    if a.ngram:
        return ngram_leg(a)
    import torch
    from dots_ocr_amd.config import DotsConfig
    from dots_ocr_amd.engine import Engine, SamplingParams
    eng = Engine(DotsConfig.tiny(), max_batch=4, max_seq_len=512, max_patches=256, max_prefill_tokens=256)
    rng = np.random.default_rng(0)
    B_max = max(a.rows)
    logits = rng.normal(0.0, 2.0, (B_max, V)).astype(np.float32)
    for b in range(B_max):
        logits[b, rng.choice(V, 64, replace=False)] = rng.uniform(8.0, 14.0, 64)
    n_prompt, n_gen = 1200, 300
    hist = rng.integers(0, V, (B_max, n_prompt + n_gen)).astype(np.int32)
    d_l = torch.from_numpy(logits).cuda()
    d_h = torch.from_numpy(hist).cuda()
    d_n = torch.full((B_max,), n_prompt + n_gen, dtype=torch.int32, device="cuda")
    d_p = torch.full((B_max,), n_prompt, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    greedy = SamplingParams()
    legacy = SamplingParams(temperature=0.7, top_p=0.9, seed=1)
    loaded = [SamplingParams(temperature=0.1, top_p=0.9, top_k=50, repetition_penalty=1.1, frequency_penalty=0.2, presence_penalty=0.2, seed=b)
              for b in range(B_max)]
    cases = [("argmax", 0, lambda B: [greedy] * B), ("sampler", 1, lambda B: [legacy] * B),
             ("rows_greedy", 2, lambda B: [greedy] * B), ("rows_loaded", 2, lambda B: loaded[:B])]
    if a.rules:
        import time
        from dots_ocr_amd.engine import LogitRules
        eng.set_eos([151643, 151645])
        rules = []
        for b in range(B_max):
            allowed = rng.choice(V, 5000, replace=False)
            allowed[:64] = np.argsort(-logits[b])[:64]                # the peaked head stays selectable
            allowed = sorted(set(int(x) for x in allowed))
            bias = {int(t): float(v) for t, v in zip(allowed[:300], rng.uniform(-2.0, 2.0, 300))}
            rules.append(LogitRules(bias=bias, allowed=allowed, min_tokens=10 ** 6, stop=allowed[300:304]))
        for B in a.rows:
            for name, params in (("rows_greedy", [greedy] * B), ("rows_loaded", loaded[:B])):
                for tag, rl in (("", [None] * B), ("+rules", rules[:B])):
                    ms = eng.bench_select_tokens_rules(d_l.data_ptr(), B, V, params, rl, None, d_h.data_ptr(), d_n.data_ptr(), n_prompt + n_gen,
                                                       d_p.data_ptr(), a.iters)
                    print(json.dumps({"rows": B, "V": V, "stage": name + tag, "us": round(ms * 1e3, 2), "iters": a.iters}), flush=True)
        eng.close()
        # setting a row's rules on an engine of the real vocabulary width (no weights needed: only the selection state is touched)
        big = Engine(DotsConfig.tiny(vocab=V), max_batch=4, max_seq_len=512, max_patches=256, max_prefill_tokens=256)
        big.set_row_logit_rules(0, rules[0])                             # first call: allocates the state
        big.synchronize()
        t0 = time.perf_counter()
        for i in range(50):
            big.set_row_logit_rules(i % 4, rules[i % B_max])
        t1 = time.perf_counter()
        big.synchronize()
        t2 = time.perf_counter()
        print(json.dumps({"stage": "set_row_logit_rules", "V": V, "bias": 300, "allowed": len(rules[0].allowed), "host_us_per_call": round((t1 - t0) / 50 * 1e6, 1),
                          "with_final_sync_us_per_call": round((t2 - t0) / 50 * 1e6, 1)}), flush=True)
        big.close()
        return
    for B in a.rows:
        for name, mode, params in cases:
            ms = eng.bench_select_tokens(d_l.data_ptr(), B, V, params(B), d_h.data_ptr(), d_n.data_ptr(), n_prompt + n_gen, d_p.data_ptr(),
                                         mode, a.iters)
            print(json.dumps({"rows": B, "V": V, "stage": name, "us": round(ms * 1e3, 2), "iters": a.iters}), flush=True)
    eng.close()


def guided_leg(a):
    import time
    import torch
    from dots_ocr_amd import guided as G
    from dots_ocr_amd.config import DotsConfig
    from dots_ocr_amd.engine import Engine, LogitRules, SamplingParams
    eng = Engine(DotsConfig.tiny(vocab=V), max_batch=4, max_seq_len=512, max_patches=256, max_prefill_tokens=256)
    rng = np.random.default_rng(0)
    # a byte-level vocabulary: the 256 bytes, then 1..12-byte pieces of JSON-looking and plain text (what a BPE vocabulary is made of)
    pieces = [bytes([c]) for c in b'0123456789 ,:[]{}"\n-.abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ'] + ["é".encode(), "中".encode()]
    toks = [bytes([i]) for i in range(256)]
    toks += [b"".join(pieces[int(j)] for j in rng.integers(0, len(pieces), int(rng.integers(1, 7)))) for _ in range(256, V)]
    eos = [151643, 151645]
    eng.set_eos(eos)
    eng.set_token_bytes(G.TokenBytes(toks, eos))
    t0 = time.perf_counter()
    guide = G.compile_json_schema(G.layout_schema())
    t1 = time.perf_counter()
    h = eng.create_guide(guide)
    t2 = time.perf_counter()
    for _ in range(20):
        eng.destroy_guide(eng.create_guide(guide))
    t3 = time.perf_counter()
    print(json.dumps({"stage": "guide_create", "states": guide.n_states, "compile_ms": round((t1 - t0) * 1e3, 1), "first_create_us": round((t2 - t1) * 1e6, 1),
                      "create_destroy_us": round((t3 - t2) / 20 * 1e6, 1)}), flush=True)
    prefixes = [b"", b"[", b'[{"bbox": [12, 3', b'[{"bbox": [1, 2, 3, 4], "category": "', b'[{"bbox": [1, 2, 3, 4], "category": "Text", "text": "ab',
                b'[{"bbox": [1, 2, 3, 4], "category": "Text"}, ', b"[]"]
    B_max = max(a.rows)
    states = [guide.walk(guide.start, prefixes[b % len(prefixes)]) for b in range(B_max)]
    logits = rng.normal(0.0, 2.0, (B_max, V)).astype(np.float32)
    for b in range(B_max):
        logits[b, rng.choice(V, 64, replace=False)] = rng.uniform(8.0, 14.0, 64)
    n_prompt, n_gen = 1200, 300
    hist = rng.integers(0, V, (B_max, n_prompt + n_gen)).astype(np.int32)
    d_l, d_h = torch.from_numpy(logits).cuda(), torch.from_numpy(hist).cuda()
    d_n = torch.full((B_max,), n_prompt + n_gen, dtype=torch.int32, device="cuda")
    d_p = torch.full((B_max,), n_prompt, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    greedy = SamplingParams()
    loaded = [SamplingParams(temperature=0.1, top_p=0.9, top_k=50, repetition_penalty=1.1, frequency_penalty=0.2, presence_penalty=0.2, seed=b)
              for b in range(B_max)]
    rules = []
    for b in range(B_max):
        allowed = sorted(set(int(x) for x in rng.choice(V, 5000, replace=False)))
        rules.append(LogitRules(bias={int(t): float(v) for t, v in zip(allowed[:300], rng.uniform(-2.0, 2.0, 300))}, allowed=allowed,
                                min_tokens=10 ** 6, stop=allowed[300:304]))
    for B in a.rows:
        for name, params in (("rows_greedy", [greedy] * B), ("rows_loaded", loaded[:B])):
            for tag, gl, rl in (("", [None] * B, [None] * B), ("+guide(1)", [h] + [None] * (B - 1), [None] * B), ("+guide(all)", [h] * B, [None] * B),
                                ("+rules(all)", [None] * B, rules[:B])):
                if B == 1 and tag == "+guide(1)":
                    continue
                ms = eng.bench_select_tokens_guided(d_l.data_ptr(), B, V, params, rl, None, gl, states[:B], d_h.data_ptr(), d_n.data_ptr(),
                                                    n_prompt + n_gen, d_p.data_ptr(), a.iters)
                print(json.dumps({"rows": B, "V": V, "stage": name + tag, "us": round(ms * 1e3, 2), "iters": a.iters}), flush=True)
    eng.set_row_guide(0, h)                                              # first call: allocates the state
    eng.synchronize()
    t0 = time.perf_counter()
    for i in range(50):
        eng.set_row_guide(i % 4, h)
    t1 = time.perf_counter()
    eng.synchronize()
    t2 = time.perf_counter()
    print(json.dumps({"stage": "set_row_guide", "host_us_per_call": round((t1 - t0) / 50 * 1e6, 1),
                      "with_final_sync_us_per_call": round((t2 - t0) / 50 * 1e6, 1)}), flush=True)
    eng.close()


def ngram_leg(a):
    import time
    import torch
    from dots_ocr_amd.config import DotsConfig
    from dots_ocr_amd.engine import Engine, NgramRule, SamplingParams
    eng = Engine(DotsConfig.tiny(), max_batch=4, max_seq_len=512, max_patches=256, max_prefill_tokens=256)
    rng = np.random.default_rng(0)
    B_max = max(a.rows)
    logits = rng.normal(0.0, 2.0, (B_max, V)).astype(np.float32)
    for b in range(B_max):
        logits[b, rng.choice(V, 64, replace=False)] = rng.uniform(8.0, 14.0, 64)
    d_l = torch.from_numpy(logits).cuda()
    n_prompt = 1200
    greedy = SamplingParams()
    loaded = [SamplingParams(temperature=0.1, top_p=0.9, top_k=50, repetition_penalty=1.1, frequency_penalty=0.2, presence_penalty=0.2, seed=b)
              for b in range(B_max)]
    for n_gen in (64, 1024, 16384):
        stride = n_prompt + n_gen
        for kind in ("random", "loop"):
            hist = rng.integers(0, V, (B_max, stride)).astype(np.int32)
            if kind == "loop":
                hist[:, n_prompt:] = hist[:, n_prompt:n_prompt + 7][:, np.arange(n_gen) % 7]
            d_h = torch.from_numpy(hist).cuda()
            d_n = torch.full((B_max,), stride, dtype=torch.int32, device="cuda")
            d_p = torch.full((B_max,), n_prompt, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            for B in a.rows:
                for name, params in (("rows_greedy", [greedy] * B), ("rows_loaded", loaded[:B])):
                    for tag, rule in (("", None), ("+ngram(n=30,W=90)", NgramRule(30, 90)), ("+ngram(n=30,W=0)", NgramRule(30, 0))):
                        if rule is not None and n_gen < rule.window:
                            continue                                     # the window would reach past the history: same as W = 0
                        ms = eng.bench_select_tokens_ngram(d_l.data_ptr(), B, V, params, [None] * B, [rule] * B, d_h.data_ptr(), d_n.data_ptr(), stride,
                                                           d_p.data_ptr(), a.iters)
                        print(json.dumps({"rows": B, "V": V, "history": n_gen, "kind": kind, "stage": name + tag, "us": round(ms * 1e3, 2),
                                          "iters": a.iters}), flush=True)
    eng.close()
    big = Engine(DotsConfig.tiny(vocab=V), max_batch=4, max_seq_len=512, max_patches=256, max_prefill_tokens=256)
    rule = NgramRule(30, 90, tuple(range(16)))
    big.set_row_ngram(0, rule)                                           # first call: allocates the state
    big.synchronize()
    t0 = time.perf_counter()
    for i in range(50):
        big.set_row_ngram(i % 4, rule)
    t1 = time.perf_counter()
    big.synchronize()
    t2 = time.perf_counter()
    print(json.dumps({"stage": "set_row_ngram", "V": V, "host_us_per_call": round((t1 - t0) / 50 * 1e6, 1),
                      "with_final_sync_us_per_call": round((t2 - t0) / 50 * 1e6, 1)}), flush=True)
    big.close()


if __name__ == "__main__":
    main()
