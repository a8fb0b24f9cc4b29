"""Sensitivity gates of the terminal-enforcing GPU parity tests (tests/test_gpu_terminal.py), on the fp64
oracle alone: for every net those tests use, at the oracle's own points of the same counters,

  (a) the ansatz matters: the labels with the ansatz differ from those with the bare inner network N
      (OnlyGradient: from the plain head net's) by rel-L2 >= 1e-2 on the value column and on the gradient
      block;
  (b) the net matters: they differ from the labels of the ansatz around an all-zero N by rel-L2 >= 1e-3
      on the value column and >= 1e-2 on the gradient block.

A kernel that dropped g, grad g or the (T - t) factor fails parity by (a); one that dropped N by (b).
The scale factors that make both hold are tests/terminal_util.py SCALES.  CPU, fp64."""
import numpy as np
import pytest

import terminal_util as T
from oracle import dpi_oracle as O


def test_case_set():
    """Cha and OU x Value and OnlyGradient x ELU and Tanh x six width shapes at nx = 7; two of the shapes,
    with both activations, also at nx = 100 and 128."""
    at7 = {c[:4] for c in T.GPU_CASES if c[4] == 7}
    assert len(at7) == 2 * 2 * 2 * 6 and {c[3] for c in at7} == set(T.WIDTHS)
    for nx in (100, 128):
        assert {c[:4] for c in T.GPU_CASES if c[4] == nx} == {
            (e, k, a, w) for e in ("cha", "ou") for k in ("Value", "OnlyGradient") for a in ("ELU", "Tanh")
            for w in ("w64x4", "w256x8")}
    assert len(T.GPU_CASES) == len(set(T.GPU_CASES)) == 48 + 32


@pytest.mark.parametrize("case", T.GPU_CASES, ids=T.case_id)
def test_gates(case):
    eq_kind, kind, act, wtag, nx = case
    oeq = T.oracle_equation(eq_kind, nx)
    module, acts = T.case_nets(*case)
    twin = T.from_module(oeq, module, acts, kind)
    tx = np.asarray(O.sample_points(oeq, T.N, T.SEED, T.EPOCH, 0), np.float64)
    ref, a, b = T.gate_parts(oeq, twin, tx)
    print(T.case_id(case), "(a)", a, "(b)", b)
    assert np.isfinite(ref).all()
    T.assert_gates(a, b, T.case_id(case))
