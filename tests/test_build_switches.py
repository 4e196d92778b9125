"""DESIGN.md's table of compile-time switches (section 6.1) names exactly the
identifiers that the kernel sources test with #if / #ifdef / #ifndef / #elif:
an experiment switch is written down there or removed."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ggml-cuda-experiments_amd", "csrc")
_NOT_NAMES = {"defined"}


def switches_in_sources():
    names = set()
    for path in glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(CSRC, "*.hip")):
        with open(path) as f:
            text = f.read().replace("\\\n", " ")
        for cond in re.findall(r"^[ \t]*#[ \t]*(?:if|ifdef|ifndef|elif)\b(.*)$", text, re.M):
            cond = re.sub(r"//.*|/\*.*?\*/", "", cond)
            names |= set(re.findall(r"\b[A-Za-z_]\w*", cond)) - _NOT_NAMES
    return names


def switches_in_design():
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        text = f.read()
    section = text.split("### 6.1 Compile-time switches", 1)[1].split("\n**Retired switches.**", 1)[0]
    rows = [l for l in section.splitlines() if l.startswith("| `")]
    return [re.match(r"\| `(\w+)` \|", l).group(1) for l in rows]


def test_design_table_names_every_switch_of_the_sources():
    table = switches_in_design()
    assert len(table) == len(set(table)), "a switch is listed twice"
    src = switches_in_sources()
    assert src, "no conditional found: the scan is broken"
    assert set(table) == src, {"only in DESIGN.md": sorted(set(table) - src), "only in csrc": sorted(src - set(table))}
