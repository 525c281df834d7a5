"""The dynamic-LDS opt-in follows the size a launch asks for (csrc/launch.h ensure_dyn_lds): a kernel whose LDS depends on a run-time
dimension, launched first at a small and then at a larger dimension in ONE process, has to be opted in again for the larger size.  The
opt-in state is per process, so the four launches run in a fresh child (tests/lds_optin_worker.py, which states the shapes and what
each result is compared with) that no earlier test has raised the opt-in of."""
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent


def test_lds_optin_is_raised_when_a_later_launch_needs_more():
    p = subprocess.run([sys.executable, str(ROOT / "tests" / "lds_optin_worker.py")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = p.stdout.splitlines()
    assert [ln for ln in lines if ln.startswith("returned: ")] == [
        "returned: gateup B=17 H=768", "returned: gateup B=17 H=1536", "returned: proj B=1 N=16 K=3584", "returned: proj B=1 N=16 K=8960"], p.stdout
    assert sorted(ln for ln in lines if ln.startswith("ok: ")) == ["ok: gateup H=1536", "ok: gateup H=768", "ok: proj K=3584", "ok: proj K=8960"], p.stdout
