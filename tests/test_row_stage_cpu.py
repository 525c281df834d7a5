"""RowStage (csrc/row_stage.h), the host record of which rows the per-row selection stage owns: the exhaustive model check of
tests/row_stage_model.cpp, compiled with the system C++ compiler and run (no GPU, no HIP)."""
import re
import shutil
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "dots_ocr_amd" / "csrc"
ENGINE_SOURCES = ("engine.h", "engine.hip", "weights.hip", "slots.hip", "rows.hip", "ops.hip")      # the engine's host code


def test_row_stage_matches_brute_force_model(tmp_path):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no C++ compiler (c++, g++ or clang++) on PATH"
    max_batch = re.search(r"^#define DOTS_MAX_BATCH (\d+)", (CSRC / "kernels.h").read_text(), re.M).group(1)
    exe = tmp_path / "row_stage_model"
    cmd = [cxx, "-std=c++17", "-O2", "-Wall", f"-DDOTS_MAX_BATCH={max_batch}", f"-I{CSRC}",
           str(ROOT / "tests" / "row_stage_model.cpp"), "-o", str(exe)]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    # every sequence of 1 .. 6 operations out of 10, walked twice (alone and beside a second row)
    n_ops = int(re.search(r"(\d+) operations", p.stdout).group(1))
    assert n_ops == 2 * sum(10 ** k for k in range(1, 7)), p.stdout


def test_engine_keeps_no_second_copy_of_stage_membership():
    """The counters and flag arrays RowStage replaced stay gone from the engine, and so does the hand-written conjunction over them."""
    src = "".join((CSRC / f).read_text() for f in ENGINE_SOURCES)
    for gone in ("row_own[", "row_rules[", "row_ngram[", "n_own", "n_rules", "n_guided", "n_ngram", "n_stop_rows"):
        assert not re.search(r"\b" + re.escape(gone), src), gone
    assert not re.search(r"!e->row_\w+\[\w+\]\s*&&", src)
    # one statement of what the stage launches: the step and the single-kernel entry points both go through launch_row_stage
    for launcher in ("launch_select_rows(", "launch_ngram_ban(", "launch_guide_mask("):
        assert src.count(launcher) == 1, launcher
