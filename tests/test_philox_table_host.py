"""The table form of Philox4x32-10 (csrc/dpi_rng.h: philox_table_entry + philox_lane_invariant +
philox4x32_10_tail, what the first-order rollouts run) against oracle/philox.py, on the host: a
stand-alone program compiled with hipcc from the header prints the four output words of a list of
counters.  No GPU."""
import itertools
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from oracle import philox as PH

ROOT = Path(__file__).resolve().parents[1]
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def counters():
    nb, K = 25, 50  # nx = 100, K = 50: the workload's largest c0 is K nb - 1
    c0s = [0, 1, K * nb - 1, 2**32 - 1]
    ms = [0, 63, 4095, 2**32 - 1]
    pts = [0, 1, 15, 4096, 2**32 - 1]
    c3s = [PH.c3_word(PH.TAG_TERM, 3), PH.c3_word(PH.TAG_INT, 3), PH.c3_word(PH.TAG_INT, 0xABCDEF)]
    seeds = [(5 << 32) | 1, 0xDEADBEEF12345678]
    rows = list(itertools.product(c0s, ms, pts, c3s, seeds))
    rng = np.random.default_rng(0)  # and every step of a rollout, with random other words
    for k in range(K * nb):
        rows.append((k, int(rng.integers(0, 2**32)), int(rng.integers(0, 2**32)), c3s[k % 3], seeds[k % 2]))
    return rows


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    if not Path(HIPCC).exists():
        pytest.fail(f"hipcc not found ({HIPCC})")
    exe = tmp_path_factory.mktemp("philox_host") / "philox_table_host"
    subprocess.run([HIPCC, "--offload-host-only", "-O1", "-std=c++17", "-o", str(exe),
                    str(ROOT / "tests" / "philox_table_host.hip")], check=True)
    return exe


def test_table_form_words_equal_the_oracle(prog):
    rows = counters()
    assert len(rows) > 1000
    text = "".join(f"{c0} {m} {i} {c3} {s & 0xFFFFFFFF} {s >> 32}\n" for c0, m, i, c3, s in rows)
    out = subprocess.run([str(prog)], input=text, capture_output=True, text=True, check=True).stdout
    got = np.array([[int(w) for w in line.split()] for line in out.splitlines()], dtype=np.uint32)
    assert got.shape == (len(rows), 4)
    for seed in sorted({r[4] for r in rows}):
        sel = [n for n, r in enumerate(rows) if r[4] == seed]
        c0, m, i, c3 = (np.array([rows[n][q] for n in sel], dtype=np.uint64) for q in range(4))
        want = np.stack(PH.philox4x32_10(c0, m, i, c3, seed), axis=-1)
        bad = np.nonzero((got[sel] != want).any(axis=1))[0]
        assert bad.size == 0, f"seed {seed:#x}: {bad.size} counters differ, first {rows[sel[bad[0]]]}"
