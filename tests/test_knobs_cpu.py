"""The environment switches the code reads are the ones DESIGN.md section 5 lists, each read at one place (plain source checks: no
library load).  The library reads the environment through mi_env_int / mi_diag_knob of csrc/common.h only; the package through os.environ."""
import glob
import os
import re
from collections import Counter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "medical_image_generation_amd")


def _csrc_sources():
    return sorted(glob.glob(os.path.join(PKG, "csrc", "*.hip")) + glob.glob(os.path.join(PKG, "csrc", "*.h")))


def _csrc_reads():
    """(name, file) of every mi_env_int("MI_...") / mi_diag_knob("MI_...") call"""
    out = []
    for path in _csrc_sources():
        for name in re.findall(r'\bmi_(?:env_int|diag_knob)\(\s*"(MI_[A-Z0-9_]+)"', open(path).read()):
            out.append((name, os.path.basename(path)))
    return out


def _python_reads():
    names = set()
    for path in glob.glob(os.path.join(PKG, "*.py")):
        names.update(re.findall(r'(?:environ(?:\.get)?\s*[\(\[]|getenv\()\s*["\'](MI_[A-Z0-9_]+)["\']', open(path).read()))
    return names


def _design_switches():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    paragraphs = [p for p in re.split(r"\n\s*\n", text) if p.startswith("**Switches**")]
    assert len(paragraphs) == 1
    return set(re.findall(r"`(MI_[A-Z0-9_]+)`", paragraphs[0]))


def test_switches_read_are_the_switches_documented():
    read = {n for n, _ in _csrc_reads()} | _python_reads()
    assert len(read) > 20  # the patterns above still find the reads
    documented = _design_switches()
    assert read == documented, f"undocumented: {sorted(read - documented)}; documented but not read: {sorted(documented - read)}"


def test_each_library_switch_is_read_at_one_site():
    twice = {n: c for n, c in Counter(n for n, _ in _csrc_reads()).items() if c > 1}
    assert not twice, twice


def test_library_reads_environment_only_in_common_h():
    for path in _csrc_sources():
        if os.path.basename(path) != "common.h":
            assert "getenv(" not in open(path).read(), path
    assert open(os.path.join(PKG, "csrc", "common.h")).read().count("getenv(") == 2  # mi_env_int, mi_diag_knob
