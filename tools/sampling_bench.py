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
    a = ap.parse_args()
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


if __name__ == "__main__":
    main()
