"""The environment switches (csrc/switches.h): the table check of tests/switches_model.cpp, compiled with the system C++ compiler — plainly
and with the address and undefined-behaviour sanitizers — and run (no GPU, no HIP); and that the header stays the only place where the
library reads the environment or spells a switch's name."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "dots_ocr_amd" / "csrc"
SOURCES = sorted(p for p in CSRC.iterdir() if p.suffix in (".hip", ".h", ".cpp", ".hpp"))


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")], ids=["plain", "asan-ubsan"])
def test_switch_rules_match_the_table(tmp_path, flags):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no C++ compiler (c++, g++ or clang++) on PATH"
    exe = tmp_path / "switches_model"
    cmd = [cxx, "-std=c++17", "-O1", "-Wall", *flags, f"-I{CSRC}", str(ROOT / "tests" / "switches_model.cpp"), "-o", str(exe)]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    m = re.search(r"(\d+) checks, 0 mismatches", p.stdout)
    assert m and int(m.group(1)) > 300, p.stdout


def test_only_switches_h_reads_the_environment():
    for src in SOURCES:
        if src.name != "switches.h":
            assert "getenv" not in src.read_text(), src.name
    assert (CSRC / "switches.h").read_text().count("getenv(") == 1             # read_now


def test_every_switch_name_is_defined_once_in_switches_h():
    header = (CSRC / "switches.h").read_text()
    defined = re.findall(r'"(DOTS_OCR_[A-Z0-9_]+)"', header)
    assert len(defined) == len(set(defined)) and len(defined) >= 30, sorted(defined)
    for name in defined:                                                        # defined means: a constant of the sw namespace holds the text
        assert re.search(r"^constexpr const char\* \w+ = \"" + name + r"\";", header, re.M), name
    for src in SOURCES:
        text = src.read_text()
        for name in re.findall(r"DOTS_OCR_[A-Z0-9_]+", text):                   # comments included: no name that switches.h does not know
            assert name in defined, f"{src.name}: {name}"
        if src.name != "switches.h":
            assert not re.search(r'"[^"\n]*DOTS_OCR_', text), f"{src.name} spells a switch name in a string"
