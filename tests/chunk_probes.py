"""Probes of the paged prefill attention kernel (csrc/attn_paged.hip): a block of m new query rows behind a prefix of c keys
that already lie in the sequence's pages.  Built from tests/attention_probes.py — indicator V, planted keys, poison behind the sequence,
the float64 reference and its tolerance are that file's; nothing here introduces a number of its own.

suffix_probe(c, m) is one causal Seq with n = c + m keys and nq = m query rows (Seq places query row r at key position r + c).
Checked rows: the first two, the last two, and the two rows on either side of every 64-position boundary inside the new rows (where one
query block / page ends and the next begins).  For every checked row at position p keys are planted, in this order of precedence (a key
carries one plant; an earlier class wins): the diagonal key p, its masked neighbour p + 1, both sides of the row's own page start, both
sides of the prefix's end (c - 1, c), key 0.  What lies behind key n - 1 in the last page is poison, K and V.

MUTANTS: the float64 reference with one defect of a paged kernel applied.  test_chunked_prefill_cpu.py shows that each lies >= MUTANT_FACTOR
x the tolerance away on the probes it applies to, and that the bf16-emulated oracle lies inside the tolerance on every probe.
"""
import copy

import torch

import attention_probes as ap

SHAPES = [(0, 1), (0, 64), (0, 65), (64, 1), (64, 64), (128, 130), (320, 64), (192, 257)]
BIG_SHAPE = (5056, 64)                        # the real model's heads (Hq 12, Hkv 2) over an 80-page context
WEIGHTS = (0.25, 0.5, 1.0)


def checked_rows(c, m):
    rows = {0, 1, m - 2, m - 1}
    for b in range((c // 64 + 1) * 64, c + m, 64):
        rows |= {b - c - 2, b - c - 1, b - c, b - c + 1}
    return sorted(r for r in rows if 0 <= r < m)


def suffix_probe(c, m, scales=None, Hq=6, Hkv=1, seed=0):
    assert c >= 0 and m >= 1 and Hq % Hkv == 0
    n, G = c + m, Hq // Hkv
    g = torch.Generator().manual_seed(7000 + 131 * c + m + seed)
    q = torch.randn(m, Hq, 128, generator=g).bfloat16()
    k = torch.randn(n, Hkv, 128, generator=g).bfloat16()
    rows = checked_rows(c, m)
    taken, a = set(), 0
    wanted = (lambda p: p, lambda p: p + 1, lambda p: p // 64 * 64 - 1, lambda p: p // 64 * 64, lambda p: c - 1, lambda p: c, lambda p: 0)
    for key_of in wanted:
        for r in rows:
            p = c + r
            j = key_of(p)
            for kv in range(Hkv):
                if 0 <= j < n and (j, kv) not in taken:
                    taken.add((j, kv))
                    ap.plant(q, k, r, j, kv * G + (a + r) % G, kv, WEIGHTS[a % 3], p + 1)
                    a += 1
    if scales is not None:
        scales = scales[:Hkv]
    return ap.Seq(q, k, rows, causal=True, tail_k=ap.poison_rows((-n) % 64, Hkv), tail_v=ap.POISON, scales=scales,
                  name=f"suffix[{c}+{m}]")


def positions(seq):
    return torch.tensor(seq.rows) + seq.n - seq.nq


# ------------------------------------------------------------------------------------------------ mutants
def _with_limits(seq, limits):
    s = copy.copy(seq)
    s.limits = limits
    return s


def _m_causal_plus(seq):
    """every row also sees the key behind its own: the next row's, and behind the last row the poison of the page's unused slots"""
    return _with_limits(seq, seq.limits + 1), dict(tail=True)


def _m_causal_minus(seq):
    return seq, dict(limit_shift=-1)


def _m_prefix_page_dropped(seq):
    c = seq.n - seq.nq
    if c < 64:
        return None
    t = c // 64 // 2
    m = torch.ones(1, seq.n, dtype=torch.float64)
    m[:, 64 * t:64 * t + 64] = 0.0
    return seq, dict(mult=m)


def _m_pages_exchanged(seq):
    """the table entries of page 0 and of a row's diagonal page exchanged: what sits in the diagonal slot is then masked past the row's
    offset in its page (modelled by that mask effect alone, as attention_probes._m_page_exchange does; the future or poisoned keys read
    in page 0's place only move the result further)"""
    pos = positions(seq)
    if int(pos.max()) < 64:
        return None
    j = torch.arange(seq.n).view(1, -1)
    gone = (pos.view(-1, 1) >= 64) & (j < 64) & (j > (pos % 64).view(-1, 1))
    return seq, dict(mult=(~gone).double())


def _m_page_unmasked(seq):
    """the page that holds a row's last visible key read unmasked to its 64th slot: the keys behind the row, and behind the last row the poison"""
    lim = (positions(seq) // 64 + 1) * 64
    return _with_limits(seq, lim), dict(tail=True)


MUTANTS = {
    "causal limit +1": _m_causal_plus,
    "causal limit -1": _m_causal_minus,
    "a prefix page dropped": _m_prefix_page_dropped,
    "two pages exchanged": _m_pages_exchanged,
    "the last page read unmasked to 64": _m_page_unmasked,
}


def mutant_output(seq, code, name):
    spec = MUTANTS[name](seq)
    if spec is None:
        return None
    s, kw = spec
    if kw.get("tail"):                         # attend() widens the mask to the tail only; the limits of _with_limits may reach into it
        kw = dict(kw)
        n, m = s.n, len(s.tail_k)
        S = s._scores()[..., :n + m]
        M = (torch.arange(n + m).view(1, -1) < s.limits.view(-1, 1)).double()
        Sm = S.masked_fill(M == 0, float("-inf"))
        P = torch.exp(Sm - Sm.max(-1, keepdim=True).values) * M
        P = P / P.sum(-1, keepdim=True)
        vv = torch.cat([s.v_ref(code).double(), torch.full((m, s.Hkv, 128), s.tail_v, dtype=torch.float64)])
        G = s.Hq // s.Hkv
        return torch.stack([P[h] @ vv[:, h // G] for h in range(s.Hq)]).transpose(0, 1).contiguous()
    return s.attend(s.v_ref(code), **kw)
