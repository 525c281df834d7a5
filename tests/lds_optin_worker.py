"""Child process of tests/test_lds_optin_gpu.py: `python tests/lds_optin_worker.py`.

In a process that has launched nothing yet, two kernels whose dynamic LDS follows a run-time dimension are launched at a small and
then at a larger dimension, each above the 64 KiB that needs an opt-in (csrc/launch.h ensure_dyn_lds):
  the two-tile gate|up kernel, 17 rows:  H = 768 -> 81 920 B,   H = 1536 -> 131 072 B      (I = 64: two pairs of 16-row weight tiles)
  dec_proj_lds_kernel, 1 row, N = 16:    K = 3584 -> 73 728 B,  K = 8960 -> 159 744 B
Every call has to return, and its result has to equal bit for bit
  gate|up:    the same rows computed in calls of at most 16 rows (the one-tile kernels);
  projection: the same call repeated afterwards with the two K in the other order,
and to lie within the tolerance of test_decode_kernels_gpu.py's oracle reference.  Prints one line per step; exit status 0 = all held."""
import math
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

import torch  # noqa: E402

import test_decode_kernels_gpu as dk  # noqa: E402  (bf, dev, close, the oracle and EPS of the decode-kernel tests)
from oracle import model as om  # noqa: E402

B_GU, I, N = 17, 64, 16


def gateup_case(H):
    g = torch.Generator().manual_seed(H)
    h, ln_w = dk.bf(torch.randn(B_GU, H, generator=g) * 3), dk.bf(1 + 0.1 * torch.randn(H, generator=g))
    gate, up = dk.bf(torch.randn(I, H, generator=g) / math.sqrt(H)), dk.bf(torch.randn(I, H, generator=g) / math.sqrt(H))
    x = om.rms_norm(h.float(), ln_w.float(), dk.EPS, True)
    ref = om._r(torch.nn.functional.silu(x @ gate.float().t()) * (x @ up.float().t()), True)
    return dict(H=H, dev=[dk.dev(t) for t in (h, ln_w, gate, up)], ref=ref)


def run_gateup(eng, c, r0, n):
    hd, lnd, gd, ud = c["dev"]
    hs = hd[r0:r0 + n].contiguous()
    out = torch.zeros(n, I, dtype=torch.bfloat16, device="cuda")
    torch.cuda.synchronize()
    eng.op_dec_gateup(hs.data_ptr(), lnd.data_ptr(), gd.data_ptr(), ud.data_ptr(), out.data_ptr(), n, c["H"], I, dk.EPS)
    eng.synchronize()
    return out


def proj_case(K):
    g = torch.Generator().manual_seed(K)
    x = dk.bf(torch.randn(1, K, generator=g))
    W = dk.bf(torch.randn(N, K, generator=g) / math.sqrt(K))
    h = dk.bf(torch.randn(1, N, generator=g) * 2)
    return dict(K=K, h=h, dev=[dk.dev(x), dk.dev(W)], ref=om._r(h.float() + x.float() @ W.float().t(), True))


def run_proj(eng, c):
    xd, Wd = c["dev"]
    hd = dk.dev(c["h"].clone())
    torch.cuda.synchronize()
    eng.op_dec_proj(xd.data_ptr(), Wd.data_ptr(), hd.data_ptr(), 1, N, c["K"])
    eng.synchronize()
    return hd


def main():
    from dots_ocr_amd.config import DotsConfig
    from dots_ocr_amd.engine import Engine
    eng = Engine(DotsConfig.tiny(), max_batch=2, max_seq_len=256, max_patches=256, max_prefill_tokens=256)
    gu = [gateup_case(768), gateup_case(1536)]
    pr = [proj_case(3584), proj_case(8960)]
    # the four launches the test is about, small dimension first, before anything else runs in this process
    for c in gu:
        c["out"] = run_gateup(eng, c, 0, B_GU)
        print(f"returned: gateup B={B_GU} H={c['H']}", flush=True)
    for c in pr:
        c["out"] = run_proj(eng, c)
        print(f"returned: proj B=1 N={N} K={c['K']}", flush=True)
    for c in gu:
        assert float(c["out"].float().abs().max()) > 0
        for r0, n in ((0, 16), (16, 1)):
            one_tile = run_gateup(eng, c, r0, n)
            assert torch.equal(c["out"][r0:r0 + n].view(torch.int16), one_tile.view(torch.int16)), f"gate|up H={c['H']} rows {r0}..{r0 + n - 1}"
        dk.close(c["out"], c["ref"], rel=2 ** -6, abs_=2e-3, what=f"gate/up H={c['H']}")
        print(f"ok: gateup H={c['H']}", flush=True)
    for c in reversed(pr):
        again = run_proj(eng, c)
        assert torch.equal(c["out"].view(torch.int16), again.view(torch.int16)), f"proj K={c['K']}"
        dk.close(c["out"], c["ref"], what=f"proj K={c['K']}")
        print(f"ok: proj K={c['K']}", flush=True)
    eng.close()


if __name__ == "__main__":
    main()
