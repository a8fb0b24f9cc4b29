"""The route (csrc/dpi_route.h: which unit serves a (problem, network) pair for one kind of call, or why
none does) against the decisions of the code it replaced.  A stand-alone program compiled from the
header (tests/route_host.hip) prints the route of every pair of its sweep, one line each with the five
kinds of call side by side, behind a legend of the refusal texts; tests/golden/route_table.txt holds the
same lines as the previous routing code answered them (profiles/route_refactor/README.md says how they
were recorded).  No GPU.

The sweep: Cha / OU / GBM at nx = 7, 128, 129, 256, TD off and on; zero nets, PISGradNet, value MLPs
from [16] to [256] x 8 with ELU and Tanh in both GEMM modes, both gradient heads and terminal-enforcing
value and head nets at both width caps (one of each built for another T), a wrong input width and a
padded width past the maximum; each as a point baseline, a path launch, a Hessian-label launch, a
fused-baseline launch and the family question.  One representative per branch: every net at nx = 7 and
129, one of each kind at 128 and 256, exact fp32 where the GEMM mode can matter."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
ROUTE_H = ROOT / "deeppicarditeration_amd" / "csrc" / "dpi_route.h"
GOLDEN = ROOT / "tests" / "golden" / "route_table.txt"


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    if not Path(HIPCC).exists():
        pytest.fail(f"hipcc not found ({HIPCC})")
    exe = tmp_path_factory.mktemp("route_host") / "route_host"
    subprocess.run([HIPCC, "--offload-host-only", "-O1", "-std=c++17", "-o", str(exe),
                    str(ROOT / "tests" / "route_host.hip")], check=True)
    return subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()


def test_route_equals_recorded_decisions(table):
    want = GOLDEN.read_text().splitlines()
    assert len(table) == len(want) <= 5000
    diff = [(g, w) for g, w in zip(table, want) if g != w]
    assert not diff, f"{len(diff)} lines differ, the first:\n{diff[0][0]}\n{diff[0][1]}"


def test_every_unit_is_reached(table):
    rows = re.findall(r"^\s*X\((\w+),", ROUTE_H.read_text(), flags=re.M)
    assert len(rows) == len(set(rows)) == 50
    seen = {u for ln in table for u in re.findall(r"unit=(\S+)", ln)}
    assert seen - {"-"} == set(rows)


def test_every_refusal_text_is_reached(table):
    src = ROUTE_H.read_text()
    block = src[src.index("// ---- refusal texts"):]
    # string literals, adjacent ones joined as the compiler joins them
    texts = ["".join(re.findall(r'"((?:[^"\\]|\\.)*)"', m.group(0)))
             for m in re.finditer(r'"(?:[^"\\]|\\.)*"(?:\s*"(?:[^"\\]|\\.)*")*', block)]
    texts = [t for t in texts if t]
    assert len(texts) >= 25
    legend = dict(ln.split(" ", 1) for ln in table if re.match(r"M\d+ ", ln))
    missing = [t for t in texts if not any(t in m for m in legend.values())]
    assert not missing, missing
    # every refusal carries one of the legend's messages, and every message is used
    calls = [c for ln in table if ln not in legend and not re.match(r"M\d+ ", ln) for c in ln.split(" | ")[2:]]
    assert len(calls) == 5 * (len(table) - len(legend))
    used = set()
    for c in calls:
        rc, m = re.search(r"rc=(-?\d+) (M\d+) ", c).groups()
        assert (rc == "0") == (m == "M0"), c
        used.add(m)
    assert used - {"M0"} == set(legend)
