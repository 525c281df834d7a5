#!/usr/bin/env python3
"""What a speculating decode step costs and what it has to accept to pay (profiles/spec_ngram.txt).

    python tools/spec_bench.py [--slots 1 8] [--k 0 1 3 7] [--steps 64] [--repeats 3] [--prompt 512] [--sampled | --guided | --shaped | --logprobs N ..]

Full-size language model with seeded random weights (the vision tower, which no text-only prompt touches, is cut to one block so that the
weights are made quickly), one engine of 64 rows.  Per slot count: the reference tokens come from an unspeculated run; then for every
k and every acceptance level the same sequences are decoded again, one step per slots_decode call, with drafts planted through
Engine.set_row_drafts before every step:

    acceptance 0     k drafts per slot, all wrong: every draft row is live (it computes and writes K/V) and none is accepted
    acceptance half  the first ceil(k / 2) drafts are the true continuation, the rest wrong
    acceptance full  all k are the true continuation

Every run is checked to reproduce the reference tokens exactly.  Reported per run (median of `repeats`, each `steps` steps, wall clock
around the loop with a final synchronise, so the per-step host work of planting the drafts is inside — it is inside for k = 0 too, which
plants nothing but pays the same one-step-per-call loop):

    ms_per_step, tokens_per_step, tokens_per_s per slot count, k and acceptance
    break_even = cost(k) / cost(0) - 1 from the acceptance-0 rows: the accepted tokens per step above which speculating is faster

--sampled (profiles/spec_sampled.txt) runs the same legs three times on engines set to Engine.set_speculation_rows(sampled=True): with
plain greedy rows, with SamplingParams(temperature=0.1, seed=...) rows (a draft row rereads its logits twice: partials and draw) and
with temperature=0.8, top_k=20, top_p=0.9 rows (four reads: partials, histogram, gather, draw).  The difference between a sampled
leg and the greedy leg at the same slots, k and acceptance is the cost of the two draft-row launches (spec_thresh_kernel,
spec_draw_kernel); the k = 0 step of a sampled leg pays the per-row selection stage instead of the arg max, as it does without speculation.

--guided (profiles/spec_guided.txt) gives every row the layout guide (guided.layout_schema) over a synthetic byte table of the full
vocabulary and runs the legs twice on one build: guided_off (Engine.set_speculation_guided(False): the guided rows verify nothing, their
draft rows idle) and guided_on.  A wrong draft is then a token the guide ALLOWS at its position where one exists (another single byte
with a transition), so that at acceptance 0 the draft rows are alive and pay the chain, the mask and the shaped arg max; `alive` is the
share of planted drafts the guide could have committed.  break_even of a guided_on row = its cost / the k = 0 cost of guided_off - 1.

--shaped (profiles/spec_shaped.txt; run it with --slots 1 2 4 8 --k 0 1 3 7) gives every row an n-gram rule (size 6, window 256), logit
rules (a bias on 16 ids, min_tokens past the run) and greedy parameters with a repetition, frequency and presence penalty, and runs the
legs twice on one build: shaped_off (Engine.set_speculation_shaped(): the rows verify nothing, their draft rows idle) and shaped_on (all
three bits, with set_speculation_rows(sampled=True) for the parameters).  A live draft row then pays the draft rows' ban kernel and the
shaped selection.  break_even of a shaped_on row = its cost / the k = 0 cost of shaped_off - 1.

--logprobs N [N ..] (profiles/spec_logprobs.txt; the record there ran --logprobs 0 5 20) switches every row's logprobs on with top_n = N
and runs the legs twice per N on one build: lpN_off (Engine.set_speculation_logprobs(False): the rows verify nothing, their draft rows
idle) and lpN_on.  A live draft row then pays the draft rows' partial pass whether or not it is accepted, an accepted one its entry.
break_even of an lpN_on row = its cost / the k = 0 cost of lpN_off - 1.

One JSON line per measurement on stdout, then a table.
"""
import argparse
import dataclasses
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
    ap.add_argument("--slots", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--k", type=int, nargs="+", default=[0, 1, 3, 7])
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--sampled", action="store_true", help="also run sampled speculating rows (2-read and 4-read parameter sets) beside the greedy leg")
    ap.add_argument("--guided", action="store_true", help="every row holds the layout guide: the legs with Engine.set_speculation_guided off and on")
    ap.add_argument("--shaped", action="store_true", help="every row carries an n-gram rule, logit rules and penalties: the legs with Engine.set_speculation_shaped off and on")
    ap.add_argument("--logprobs", type=int, nargs="+", default=None, metavar="N",
                    help="every row returns logprobs with top_n = N (0 .. 20): per N the legs with Engine.set_speculation_logprobs off and on")
    ap.add_argument("--tiny", action="store_true", help="the small-dims model instead of the full-size one (a plumbing check, not a measurement)")
    a = ap.parse_args()
    from dots_ocr_amd.config import DotsConfig
    from dots_ocr_amd.engine import Engine, LogitRules, NgramRule, SamplingParams
    from dots_ocr_amd.weights import random_state_dict
    if a.tiny:
        cfg = DotsConfig.tiny(layers=3, v_layers=1)
    else:
        cfg = DotsConfig()
        cfg = dataclasses.replace(cfg, vision=dataclasses.replace(cfg.vision, num_hidden_layers=1))
    k_max = max(a.k)
    n_tok = 2 + a.steps * (k_max + 1)                                # tokens a row may reach: the prefill's, the warm-up step's, then k + 1 per step
    seq = a.prompt + n_tok + 64
    eng = Engine(cfg, max_batch=64, max_seq_len=seq, max_patches=256, max_prefill_tokens=max(a.slots) * a.prompt)
    eng.load_state_dict(random_state_dict(cfg, seed=0, threads=16))
    eng.set_eos([])
    rng = np.random.default_rng(0)
    prompts = [rng.integers(0, cfg.vocab_size - 4096, a.prompt).astype(np.int32) for _ in range(max(a.slots))]
    results = {}
    legs = [("greedy", None)]
    guide = tb = handle = None
    if a.guided:
        if a.sampled:
            raise SystemExit("--guided and --sampled are separate measurements")
        from dots_ocr_amd import guided as G
        pieces = [b'{"', b'"bbox"', b'": ', b'"category"', b'"text"', b"Text", b"Title", b"Table", b", ", b"], ", b'"}', b"12", b"345", b"ab", b"the ", b"\n"]
        g2 = np.random.default_rng(1)
        toks = [bytes([i]) for i in range(256)]
        toks += [b"".join(pieces[int(j)] for j in g2.integers(0, len(pieces), int(g2.integers(1, 4)))) for _ in range(256, cfg.vocab_size - 4096)]
        tb = G.TokenBytes(toks + [b""] * (cfg.vocab_size - len(toks)))          # the top 4096 ids: specials without bytes
        guide = G.compile_json_schema(G.layout_schema())
        eng.set_token_bytes(tb)
        handle = eng.create_guide(guide)
        legs = [("guided_off", None), ("guided_on", None)]
    if a.shaped:
        if a.sampled or a.guided:
            raise SystemExit("--shaped, --guided and --sampled are separate measurements")
        legs = [("shaped_off", None), ("shaped_on", None)]
    lp_of = {}                                                       # leg -> top_n (--logprobs)
    if a.logprobs is not None:
        if a.sampled or a.guided or a.shaped:
            raise SystemExit("--logprobs, --shaped, --guided and --sampled are separate measurements")
        if any(not 0 <= n <= 20 for n in a.logprobs):
            raise SystemExit("--logprobs takes top_n values in [0, 20]")
        legs = []
        for n in a.logprobs:
            legs += [(f"lp{n}_off", None), (f"lp{n}_on", None)]
            lp_of[f"lp{n}_off"] = lp_of[f"lp{n}_on"] = n
    alive = [0, 0]                                                   # planted drafts the guide could have committed / all planted (--guided)

    def guided_drafts(Tb, pos, k, true_drafts):
        """k drafts at output index pos of a guided row: the true ones, then single bytes the guide allows there (alive but wrong).
        -> (drafts, how many of them the step accepts: the leading true ones the guide could commit)"""
        d = [int(t) for t in Tb[pos:pos + k]]
        state = guide.start
        for t in Tb[:pos]:                                           # as the commit advances it: a token the guide did not allow moves nothing
            nxt = guide.walk(state, tb.token(int(t))) if tb.token(int(t)) else G.DEAD
            state = state if nxt == G.DEAD else nxt
        acc = 0
        for j in range(min(true_drafts, len(d))):
            state = guide.walk(state, tb.token(d[j])) if state != G.DEAD and tb.token(d[j]) else G.DEAD
            acc += state != G.DEAD and acc == j
        alive[0] += acc - min(true_drafts, len(d))                   # true drafts behind a dead one (the all -inf fallback) are dead too
        for j in range(true_drafts, len(d)):
            ok = [c for c in range(256) if state != G.DEAD and guide.table[state, c] != G.DEAD and c != d[j]]
            d[j] = ok[0] if ok else (d[j] + 1) % 256
            state = guide.walk(state, bytes([d[j]])) if ok else G.DEAD
            alive[0] += bool(ok)
        alive[0] += min(true_drafts, len(d))
        alive[1] += len(d)
        return d, acc
    if a.sampled:
        legs += [("T0.1", dict(temperature=0.1)), ("T0.8_k20_p0.9", dict(temperature=0.8, top_k=20, top_p=0.9))]
    for leg, params in legs:
      for S in a.slots:
          if any(S * (k + 1) > 64 for k in a.k):
              raise SystemExit(f"{S} slots x (k + 1) rows exceed the 64 rows of a step")
          slots = list(range(S))

          def set_rows():
              """the leg's parameters on every slot (a release clears them): row b draws with seed 1000 + b"""
              if params is not None:
                  for b in slots:
                      eng.set_row_sampling(b, SamplingParams(seed=1000 + b, **params))
              if a.guided:
                  for b in slots:
                      eng.set_row_guide(b, handle)
              if a.shaped:
                  for b in slots:
                      eng.set_row_sampling(b, SamplingParams(temperature=0.0, repetition_penalty=1.05, frequency_penalty=0.1, presence_penalty=0.1))
                      eng.set_row_logit_rules(b, LogitRules(bias={1000 + 7 * i + b: 0.5 for i in range(16)}, min_tokens=n_tok + 1, vocab_size=cfg.vocab_size))
                      eng.set_row_ngram(b, NgramRule(6, 256))
              if leg in lp_of:
                  for b in slots:
                      eng.set_row_logprobs(b, lp_of[leg])

          def run(k, true_drafts, T=None):
              """`steps` steps with k drafts per slot of which the first true_drafts are right: (seconds, tokens committed, token lists)"""
              eng.slots_reset()
              eng.set_speculation(k, 2, 0)
              eng.set_speculation_rows(sampled=a.sampled or a.shaped)
              if a.guided:
                  eng.set_speculation_guided(leg == "guided_on")
              if a.shaped:
                  on = leg == "shaped_on"
                  eng.set_speculation_shaped(ngram=on, rules=on, penalties=on)
              if leg in lp_of:
                  eng.set_speculation_logprobs(leg.endswith("_on"))
              set_rows()
              eng.slots_prefill(slots, np.concatenate(prompts[:S]), [a.prompt] * S, [n_tok] * S)
              eng.slots_decode(1)                                       # the captured step exists before the clock starts
              eng.synchronize()
              _, lens = eng.slots_poll()
              start = [int(lens[b]) for b in slots]
              pos = list(start)
              verifies = leg != "shaped_off" and not (leg in lp_of and leg.endswith("_off"))      # shaped_off and lpN_off rows verify nothing
              gain = [[1 + (min(true_drafts, k) if k and verifies else 0)] * S for _ in range(a.steps)]      # tokens a step commits per slot
              plan = None
              if a.guided and k:                                         # the automaton walks stay outside the clock
                  plan, at = [], list(start)
                  for i in range(a.steps):
                      made = [guided_drafts(T[b], at[b], k, true_drafts) for b in slots]
                      plan.append([m[0] for m in made])
                      gain[i] = [1 + (m[1] if leg == "guided_on" else 0) for m in made]      # guided_off rows verify nothing
                      at = [at[b] + gain[i][b] for b in slots]
              t0 = time.perf_counter()
              for i in range(a.steps):
                  for b in slots:
                      if k:
                          if plan is not None:
                              d = plan[i][b]
                          else:
                              d = [int(t) for t in T[b][pos[b]:pos[b] + k]]
                              d = d[:true_drafts] + [(t + 1) % (cfg.vocab_size - 4096) for t in d[true_drafts:]]
                          eng.set_row_drafts(b, d)
                      pos[b] += gain[i][b]
                  eng.slots_decode(1)
              eng.synchronize()
              dt = time.perf_counter() - t0
              _, lens = eng.slots_poll()
              toks = [eng.slot_read(b, int(lens[b])).tolist() for b in slots]
              assert [int(lens[b]) for b in slots] == pos, (k, true_drafts, [int(lens[b]) for b in slots], pos)
              if T is not None:
                  assert all(toks[b] == T[b][:len(toks[b])] for b in slots), "a speculating run left the reference tokens"
              for b in slots:
                  eng.slot_release(b)
              return dt, sum(pos) - sum(start), toks

          # reference tokens: unspeculated, as many as the fastest run will need
          eng.slots_reset()
          eng.set_speculation(0)
          set_rows()
          eng.slots_prefill(slots, np.concatenate(prompts[:S]), [a.prompt] * S, [n_tok] * S)
          for _ in range(-(-n_tok // 16)):
              eng.slots_decode(16)
          _, lens = eng.slots_poll()
          T = [eng.slot_read(b, int(lens[b])).tolist() for b in slots]
          assert all(len(t) == n_tok for t in T)
          for b in slots:
              eng.slot_release(b)
          for k in a.k:
              levels = [("-", 0)] if k == 0 else [("0", 0), ("half", -(-k // 2)), ("full", k)]
              for name, true_drafts in levels:
                  runs = [run(k, true_drafts, T) for _ in range(a.repeats)]
                  dt = statistics.median(r[0] for r in runs)
                  share = round(alive[0] / alive[1], 3) if alive[1] else None
                  alive[0] = alive[1] = 0
                  rec = {"leg": leg, "slots": S, "k": k, "rows": S * (k + 1), "acceptance": name, "steps": a.steps, "ms_per_step": round(dt / a.steps * 1e3, 4),
                         "ms_per_step_min_max": [round(min(r[0] for r in runs) / a.steps * 1e3, 4), round(max(r[0] for r in runs) / a.steps * 1e3, 4)],
                         "tokens_per_step": round(runs[0][1] / a.steps / S, 3), "tokens_per_s": round(runs[0][1] / dt, 1)}
                  if a.guided:
                      rec["alive"] = share
                  results[(leg, S, k, name)] = rec
                  print(json.dumps(rec), flush=True)
    print()
    print(f"{'leg':>14} {'slots':>5} {'k':>2} {'rows':>4} {'accept':>6} {'ms/step':>9} {'tok/step/slot':>13} {'tokens/s':>10} {'break-even accepted/step':>25}")
    for (leg, S, k, name), r in results.items():
        base = results.get(("guided_off" if a.guided else "shaped_off" if a.shaped else f"lp{lp_of[leg]}_off" if leg in lp_of else leg, S, 0, "-"))
        be = ""
        if k and name == "0" and base:
            be = f"{r['ms_per_step'] / base['ms_per_step'] - 1:.3f}"
        print(f"{leg:>14} {S:>5} {k:>2} {r['rows']:>4} {name:>6} {r['ms_per_step']:>9.4f} {r['tokens_per_step']:>13.3f} {r['tokens_per_s']:>10.1f} {be:>25}")
    eng.close()


if __name__ == "__main__":
    main()
