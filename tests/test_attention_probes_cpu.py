"""The attention probes judged WITHOUT a GPU (tests/attention_probes.py): for every probe configuration test_attention_probes_gpu.py runs,
  (a) the oracle's emulated attention (bf16 P, fp32 row sum, bf16 output) lies inside the tolerance of the fp64 reference — the tolerance is
      pinned to the reference, not to a kernel — with REL_TOL at least 3 x the measured deviation and at most MAX_EXCLUDED of the elements
      excluded as 0 < mass < FLOOR;
  (b) every applicable mutant of attention_probes.MUTANTS lies OUTSIDE the tolerance on at least one checked element, by a factor >= 4.
So a kernel that drops a tile, a page, a key or a split, shifts the causal mask, forgets the V^T group order or reads past ctx cannot pass
the GPU file.  Run with -s for the table (probe, mutant, distance / tolerance).

The last test reproduces the gap these probes close: with iid randn q, k, v and the long-context tests' tolerance
4e-3 + 2^-6 max|ref|, a dropped ragged tile / one skipped tile at 19 824 keys and a dropped ragged page at 5 201 keys go unseen."""
import pytest
import torch

import attention_probes as ap
from oracle import model as om


def emulated(seq, code):
    G = seq.Hq // seq.Hkv
    K = seq.k_ref.transpose(0, 1).repeat_interleave(G, 0)
    V = seq.v_ref(code).transpose(0, 1).repeat_interleave(G, 0)
    qs = seq.q[seq.rows].float().transpose(0, 1)
    if not seq.causal:
        return om._attention(qs, K, V, ap.SCALE, False, True).transpose(0, 1)
    out = [om._attention(qs[:, i:i + 1], K[:, :lim], V[:, :lim], ap.SCALE, False, True) for i, lim in enumerate(seq.limits.tolist())]
    return torch.cat(out, 1).transpose(0, 1)


CONFIGS = ([("prefill", n, None) for n in ap.PREFILL_PROBES] + [("causal", n, None) for n in ap.CAUSAL_PROBES]
           + [("decode", n, None) for n in ap.DECODE_PROBES] + [("decode", n, s) for n in ap.DECODE_PROBES for s in ap.KV8_SCALES])


@pytest.mark.parametrize("kind,name,scales", CONFIGS, ids=[f"{k}-{n}" + (f"-kv8_{s}" if s else "") for k, n, s in CONFIGS])
def test_probe_is_pinned_to_fp64_and_sees_every_mutant(kind, name, scales):
    seqs = ap.build(kind, name, scales)
    refs = {(i, code): seq.reference(code) for i, seq in enumerate(seqs) for code in ap.CODES}
    # (a)
    worst_rel, n_low, n_all = 0.0, 0.0, 0
    for (i, code), ref in refs.items():
        ratio, excluded, rel = ap.deviation(emulated(seqs[i], code), ref)
        assert ratio <= 1.0, f"{name} {seqs[i].name} {code}: the emulated oracle is {ratio:.2f} x the tolerance from fp64"
        worst_rel = max(worst_rel, rel)
        n_low += excluded * ref.numel()
        n_all += ref.numel()
    print(f"\n{kind} {name} {scales or ''}: emulated oracle vs fp64 {worst_rel:.5f} relative, excluded {n_low / n_all:.4f} of {n_all} elements")
    assert 3 * worst_rel <= ap.REL_TOL * 1.001, f"REL_TOL {ap.REL_TOL} is less than 3 x the measured deviation {worst_rel:.5f}"
    assert n_low / n_all <= ap.MAX_EXCLUDED
    # (b)
    for mutant, fn in ap.MUTANTS.items():
        best, seen_by = None, ""
        for (i, code), ref in refs.items():
            spec = fn(seqs[i])
            if spec is None:
                continue
            d = ap.deviation(seqs[i].attend(seqs[i].v_ref(code), **spec), ref)[0]
            if best is None or d > best:
                best, seen_by = d, f"{code} code, {seqs[i].name}"
        if best is None:
            continue
        print(f"  | {kind} {name} {scales or ''} | {mutant} | {min(best, 9999.0):.1f} | {seen_by}")
        assert best >= ap.MUTANT_FACTOR, f"{name}: mutant '{mutant}' is only {best:.2f} x the tolerance away: the probe would not see it"


@pytest.mark.parametrize("n,tail,what", [(19824, 48, "ragged"), (19824, 64, "interior"), (5201, 17, "ragged")])
def test_iid_randn_inputs_do_not_see_a_dropped_tile(n, tail, what):
    """The gap, reproduced: the long-context tests' inputs and tolerance, the emulated oracle with one defect applied (one head, 10 rows,
    5 seeds).  How large the error is depends on the draw; the mutant must pass the old check for at least one of them."""
    unseen = 0
    for seed in range(5):
        g = torch.Generator().manual_seed(seed)
        q, k, v = (torch.randn(1, m, 128, generator=g).bfloat16().float() for m in (10, n, n))
        ref = om._attention(q, k, v, ap.SCALE, False, True)
        keep = torch.ones(n, dtype=torch.bool)
        lo = n - tail if what == "ragged" else 64 * 150
        keep[lo:lo + tail] = False
        mut = om._attention(q, k[:, keep], v[:, keep], ap.SCALE, False, True)
        err, tol = float((mut - ref).abs().max()), 4e-3 + 2 ** -6 * float(ref.abs().max())
        unseen += err < tol
        print(f"\n{n} keys, seed {seed}, output std {float(ref.std()):.4f}, tolerance {tol:.4f}, {what} tile of {tail} keys never read: error {err:.4f}")
    assert unseen >= 1, "the old check sees this mutant under every draw"
