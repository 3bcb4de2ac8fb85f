"""DESIGN.md's "Run-time switches" table lists exactly the WSR_* environment variables the sources read, and the switches
of the removed conv variants are gone from the package and the tests.  A text scan: nothing is imported or built."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "gan_sr_wind_field_amd")

REMOVED = ("WSR_C1_V1", "WSR_C1_NOPF", "WSR_CT_W4", "WSR_TUNING", "WSR_CT_NARROW_WK", "WSR_CT_NARROW_M", "WSR_CT_SMALL_WK",
           "WSR_CT_SQUARE_TILES", "WSR_FWD_REGROUP", "WSR_CT_NO_MID", "WSR_FOLD_D_MASK", "WSR_CT_EPF", "WSR_CT_N16_ONEBUF")


def _files(top, exts):
    for d, _, names in os.walk(top):
        for n in names:
            if n.endswith(exts):
                yield os.path.join(d, n)


def _read(path):
    with open(path, encoding="utf-8", errors="replace") as f:
        return f.read()


def test_switch_table_matches_sources():
    read = set()
    for p in _files(os.path.join(PKG, "csrc"), (".hip", ".h")):
        read |= set(re.findall(r'WSR_ENV_(?:SET|INT|RAW)\(\s*"(WSR_[A-Z0-9_]+)"', _read(p)))
    for p in _files(PKG, (".py",)):
        read |= set(re.findall(r'environ(?:\.get\(|\[|\.pop\(|\.setdefault\()\s*"(WSR_[A-Z0-9_]+)"', _read(p)))
        read |= set(re.findall(r'"(WSR_[A-Z0-9_]+)"\s+(?:not\s+)?in\s+os\.environ', _read(p)))
    assert len(read) > 40  # (the scan found the sources)
    design = _read(os.path.join(ROOT, "DESIGN.md"))
    section = design.split("Run-time switches", 1)[1].split("\n## ", 1)[0]
    table = re.findall(r"^\| `(WSR_[A-Z0-9_]+)` \|", section, flags=re.M)
    assert len(table) == len(set(table)), sorted(n for n in set(table) if table.count(n) > 1)
    assert set(table) == read, {"read, not in the table": sorted(read - set(table)),
                                "in the table, not read": sorted(set(table) - read)}

    me = os.path.abspath(__file__)
    gone = re.compile(r"\b(" + "|".join(REMOVED) + r")\b")
    hits = []
    for top in (PKG, os.path.join(ROOT, "tests")):
        for p in _files(top, (".py", ".hip", ".h", ".md", ".ini", ".sh", ".txt", ".json", "Makefile")):
            if os.path.abspath(p) == me:
                continue
            hits += [(os.path.relpath(p, ROOT), n) for n in set(gone.findall(_read(p)))]
    assert not hits, hits
