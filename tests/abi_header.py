"""The tests' own reading of include/medimgen_hip.h, kept apart from the binding's parser (medical_image_generation_amd/_lib.py) so
that the two can disagree: names by a regex over the raw text, argument lists by a comma split of the text between the parentheses."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "include", "medimgen_hip.h")


def text() -> str:
    with open(PATH) as f:
        return f.read()


def names() -> set:
    """Every `mi_*(` of the raw text, comments included: a call-like mention of an entry point that does not exist shows up too."""
    return set(re.findall(r"\b(mi_[a-z0-9_]+)\s*\(", text()))


def params(name: str) -> list:
    """The declared parameters of `int|int64_t name(...);` as written, [] for (void).  Raises when there is no such declaration."""
    m = re.search(r"\b(?:int|int64_t) %s\s*\(([^)]*)\)\s*;" % re.escape(name), text())
    assert m, f"{name} is not declared in {PATH}"
    inner = m.group(1).strip()
    return [] if inner in ("", "void") else [p.strip() for p in inner.split(",")]
