"""The PISGradNet core alone (k_fit_core_fwd / _bwd / _wgrad of csrc/dpi_fit.h): the numpy
restatement's direct outputs sp, q, taubar, dW_l, db_l on the core's own case table against torch fp64
autograd, the cap on what an honest fp32 evaluation may be off by (the GPU test's bar is 4 x that), and the
gates that show the direct outputs see each of seven mutants.  CPU only."""
import functools

import numpy as np
import pytest
import torch

import pis_fit_reference as R

CAP = 2e-6
PAIRS = [(k, m) for k in range(len(R.CORE_CASES)) for m in R.MODES]
PAIR_IDS = [f"{R.CORE_IDS[k]}-{m}" for k, m in PAIRS]


@functools.lru_cache(maxsize=None)
def _fp64(k, mode, seed=0):
    """The restatement in fp64 on the case's fp32 inputs, upcast: computed once and never written to."""
    return R.core_outputs(R.core_case(k, mode, seed), mode)


@pytest.mark.parametrize("k,mode", PAIRS, ids=PAIR_IDS)
def test_restatement_equals_torch_fp64_autograd(k, mode):
    """sp, q, taubar and every dW_l, db_l to rel-L2 1e-12; q exists exactly where the mode forms it."""
    got, want = _fp64(k, mode), R.torch_core(R.core_case(k, mode), mode)
    names = R.core_names(k)
    assert len(got) == len(want) == len(names)
    for name, g, w in zip(names, got, want):
        assert (g is None) == (w is None) == (name == "q" and mode == "value"), name
        if g is not None:
            assert g.shape == w.shape and np.any(w), name
            assert R.rel_l2(g, w) <= 1e-12, (name, R.rel_l2(g, w))


def test_passes_keep_the_dtype_of_their_inputs():
    for mode in R.MODES:
        out = R.core_outputs(R.core_case(4, mode), mode, np.float32)  # asserts every output's dtype itself
        assert all(o is None or o.dtype == np.float32 for o in out)


@pytest.mark.parametrize("k,mode", PAIRS, ids=PAIR_IDS)
def test_fp32_evaluations_stay_under_the_cap(k, mode):
    """E_case, the largest rel-L2 of any output over torch fp32 autograd on the CPU and the restatement in
    fp32, is <= 2e-6 for seeds 0 - 2: with it the GPU test's bar 4 max(E_case, 2^-24) never exceeds 8e-6.
    Measured: at most 1.2e-6 (db_1 of (65, 1, [3]), grad, seed 1)."""
    for seed in range(3):
        inputs, want = R.core_case(k, mode, seed), _fp64(k, mode, seed)
        errs = (R.core_errors(R.torch_core(inputs, mode, torch.float32), want)
                + R.core_errors(R.core_outputs(inputs, mode, np.float32), want))
        e_case = max(e for e in errs if e is not None)
        print(f"FIT_CORE_CAP {R.CORE_IDS[k]} {mode} seed {seed} E_case {e_case:.3e}")
        assert e_case <= CAP, (seed, dict(zip(R.core_names(k) * 2, errs)))


def _n(k):
    B, nx, widths = R.CORE_CASES[k]
    return [R.NT + nx] + list(widths)  # the widths the forward's sums run over


def _applies(mutant, k, mode):
    """Whether the edge the mutant breaks is reached by case k under the mode."""
    B = R.CORE_CASES[k][0]
    if mutant in ("no_tangent", "no_v_lambdabar", "elu2_everywhere"):  # pass 3 runs
        return mode in ("grad", "q_cot_only")
    if mutant == "no_N":  # q is formed
        return mode != "value"
    if mutant == "tail_k":
        return any(n % 4 for n in _n(k))
    if mutant == "odd_row":
        return B % 2 == 1
    return mutant == "no_dtau"


def test_table_reaches_every_mutants_edge():
    assert any(c[0] % 2 == 1 and c[0] > 1 for c in R.CORE_CASES)
    assert any(_n(k)[0] % 4 for k in range(len(R.CORE_CASES)))
    assert any(n % 4 for k in range(len(R.CORE_CASES)) for n in _n(k)[1:])
    assert any(not any(n % 4 for n in _n(k)) for k in range(len(R.CORE_CASES)))  # and a case with no remainder
    for mutant in R.MUTANTS + R.CORE_MUTANTS:
        assert sum(_applies(mutant, k, m) for k, m in PAIRS) >= 4, mutant


@pytest.mark.parametrize("k,mode", PAIRS, ids=PAIR_IDS)
def test_gates(k, mode):
    """In fp64, on the direct outputs: each mutant moves the output it is about by rel-L2 >= 1e-3 wherever its
    edge is reached (no_dtau: dtau is exactly zero), and nothing at all where it is not."""
    inputs, full = R.core_case(k, mode), _fp64(k, mode)
    names = R.core_names(k)
    for mutant in R.MUTANTS + R.CORE_MUTANTS:
        got = R.core_outputs(inputs, mode, mutant=mutant)
        moved = {n: R.rel_l2(g, w) for n, g, w in zip(names, got, full) if w is not None}
        if not _applies(mutant, k, mode):
            assert not any(moved.values()), (mutant, moved)
            continue
        if mutant == "no_dtau":
            assert not np.any(got[2]) and moved["dtau"] == 1.0
            assert not any(e for n, e in moved.items() if n != "dtau")
        elif mutant == "no_N":
            assert moved["q"] >= 1e-3, (mutant, moved)
        elif mutant == "tail_k":
            assert moved["sp"] >= 1e-3, (mutant, moved)
        else:
            assert max(e for n, e in moved.items() if n[0] == "d" and n != "dtau") >= 1e-3, (mutant, moved)
            if mutant == "odd_row":  # k_fit_core_wgrad alone: the row kernels' outputs do not move
                assert not any(moved[n] for n in ("sp", "q", "dtau") if n in moved)
