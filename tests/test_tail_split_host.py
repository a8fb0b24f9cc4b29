"""The unit map of the tail units (csrc/dpi_tail_units.h) on the host: a stand-alone program compiled
from the header (tests/tail_units_host.hip) sweeps it, and prints single launches for a restatement
here.  No GPU.

The sweep (in the program, where it takes a second): every call of n nbp <= 2,048 path blocks and 64
counts above it, launched with no base blocks, with 3 and with as many as blocks, in both unit orders;
every split count for calls of up to 320 blocks, the edges of the range and the multiples of 8 around
them above — so densely for the flagship's row layout and for both nx = 128 layouts (two extra rows per
split block); the remaining layouts, which move only the rows and the cap, at sampled block counts.  It
checks that
  - the map is a bijection between grid indices and (base point | whole block | I-unit | T-unit), the
    split part in the order asked for, and the second units a suffix of the grid (the two-launch form);
  - a split block's extra rows lie inside the park, beyond the ST rows of all blocks, pairwise disjoint,
    and hold the S columns, the gst rows, bsh and an 8-byte aligned join word in that order;
  - the cap is the most that fits and reaches 0 when no row is free;
  - both units of a block have grid indices congruent mod 8 wherever the split count is a multiple of 8.
Restated here independently for a few launches: the grid order, the rows and the cap."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
PARK_ROWS, PARK_ROW_FLOATS = 2048, 8192
BASE, WHOLE, I_UNIT, T_UNIT = range(4)


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    if not Path(HIPCC).exists():
        pytest.fail(f"hipcc not found ({HIPCC})")
    exe = tmp_path_factory.mktemp("tail_units_host") / "tail_units_host"
    subprocess.run([HIPCC, "--offload-host-only", "-O2", "-std=c++17", "-o", str(exe),
                    str(ROOT / "tests" / "tail_units_host.hip")], check=True)
    return exe


def test_unit_map_sweep(prog):
    r = subprocess.run([str(prog), "sweep"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout[-2000:] + r.stderr[-2000:]
    assert int(r.stdout.split()[1]) > 100_000


def restated(nbase, nblk, want, order, nb, ng):
    """(cap, tail, [(role, block, first extra row or -1)] by grid index)."""
    floats = (nb + ng) * 256 + 64 + 2
    xr = -(-floats // PARK_ROW_FLOATS)
    cap = 0 if nblk >= PARK_ROWS else min(nblk, (PARK_ROWS - nblk) // xr)
    tail = min(want, cap)
    whole = nblk - tail
    units = [(BASE, i, -1) for i in range(nbase)] + [(WHOLE, b, -1) for b in range(whole)]
    for role in ((T_UNIT, I_UNIT) if order else (I_UNIT, T_UNIT)):
        units += [(role, whole + k, nblk + k * xr) for k in range(tail)]
    return cap, tail, units, xr


# (nbase, nblk, tail asked for, order, nb, ng)
CASES = [
    (16, 1024, 256, 0, 25, 1),    # the flagship
    (16, 1024, 5000, 1, 25, 1),   # all blocks: capped at 1,024
    (0, 1536, 1000, 0, 25, 1),    # capped by the free rows: 512
    (3, 6, 3, 1, 2, 1),
    (3, 6, 1, 0, 25, 5),          # OU: five statistics
    (0, 1024, 1024, 0, 32, 1),    # nx = 128: two extra rows per split block, cap 512
    (32, 2048, 8, 0, 25, 1),      # no free row
    (0, 2047, 8, 1, 25, 1),       # one free row
]


@pytest.mark.parametrize("case", CASES, ids=[f"{c[1]}x{c[2]}o{c[3]}nb{c[4]}" for c in CASES])
def test_unit_map_restated(prog, case):
    nbase, nblk, want, order, nb, ng = case
    out = subprocess.run([str(prog), "dump", *map(str, case)], capture_output=True, text=True, check=True).stdout
    head, *lines = out.strip().split("\n")
    h = dict(zip(head.split()[::2], map(int, head.split()[1::2])))
    cap, tail, units, xr = restated(*case)
    assert (h["cap"], h["tail"], h["grid"], h["xrows"]) == (cap, tail, nbase + nblk + tail, xr)
    assert (h["gst"], h["bsh"], h["join"]) == (nb * 256, (nb + ng) * 256, (nb + ng) * 256 + 64)
    got = [tuple(map(int, ln.split())) for ln in lines]
    assert got == [(g,) + u for g, u in enumerate(units)]
    rows = [r for (_, role, _, r) in got if role == I_UNIT]
    assert all(nblk <= r and r + xr <= PARK_ROWS for r in rows) and len(set(rows)) == len(rows)
