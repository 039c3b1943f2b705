"""The native A/B switches are declared once, in the list of activezero_amd/csrc/az_options.h.  What follows the list by hand
-- DESIGN.md's table and the routes of tests/test_gpu_switches.py -- is held to it here, and the switches that were taken
out stay out."""
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# taken out with the routes only they reached ("Switches that were taken out")
RETIRED = ["AZ_PATCH_K", "AZ_WGRAD_R16_WIDE", "AZ_CORR_FP32", "AZ_BN_BWD_FUSED", "AZ_WGRAD_FW", "AZ_CONV2D_WGRAD_W64",
           "AZ_CONV2D_ROLL_H", "AZ_CONV2D_ROLL_NT4"]


def _read(*parts):
    with open(os.path.join(REPO, *parts), encoding="utf-8") as f:
        return f.read()


def declared():
    """[(field, variable, default expression)] of AZ_OPTION_LIST"""
    text = _read("activezero_amd", "csrc", "az_options.h")
    body = text[text.index("#define AZ_OPTION_LIST(X)"):text.index("struct AzOptions")]
    return re.findall(r'^\s*X\((\w+),\s*(AZ_\w+),\s*([^,]+),\s*"[^"]*"\)', body, re.M)


def _design_table():
    """the variables named in the first column of DESIGN.md's switch table (the retired ones have a table of their own)"""
    text = _read("DESIGN.md")
    start = text.index("### A/B switches")
    table = text[start:text.index("**Switches that were taken out.**", start)]
    names = set()
    for row in table.splitlines():
        if row.startswith("| `"):
            names.update(re.findall(r"`(AZ_\w+)`", row.split("|")[1]))
    return names


def test_the_list_parses_and_holds_each_switch_once():
    rows = declared()
    assert len(rows) >= 10
    assert len(rows) == _read("activezero_amd", "csrc", "az_options.h").count("    X(")  # no row the pattern missed
    for col in (0, 1):
        assert len({r[col] for r in rows}) == len(rows)
    assert not {r[1] for r in rows} & set(RETIRED)


def test_every_declared_switch_has_a_row_in_the_design_table():
    table = _design_table()
    assert not [v for _, v, _ in declared() if v not in table]
    assert not table & set(RETIRED)


def test_every_declared_switch_is_exercised_by_the_switch_tests():
    text = _read("tests", "test_gpu_switches.py")
    assert not [v for _, v, _ in declared() if not re.search(r'"%s"' % v, text)]


def test_retired_switches_are_named_nowhere_in_the_package_or_the_tests():
    me = os.path.abspath(__file__)
    hits = []
    for top in ("activezero_amd", "tests"):
        for root, dirs, files in os.walk(os.path.join(REPO, top)):
            dirs[:] = [d for d in dirs if d not in ("__pycache__", "lib", "golden")]
            for name in files:
                path = os.path.join(root, name)
                if path == me or not name.endswith((".py", ".hip", ".h", ".cpp", ".c", ".md", ".json", ".txt")):
                    continue
                text = _read(path)
                hits += [(os.path.relpath(path, REPO), r) for r in RETIRED if re.search(r"%s(?![A-Z0-9_])" % r, text)]
    assert not hits
