"""What the host keeps per workspace (csrc/dpi_kernels.hip, the workspace tag) as a label call meets it on
the GPU: the DPI_PREPARED contract of include/dpi.h, the baseline record the fused reduce depends on, and
the launch timer of a refused call.  The pair is the smallest one whose dpi_label_prepare stages
something without PISGradNet: GBM at nx = 7 with the [32, 32] ELU net of tests/net_weight_cases.py (the
noise sums of k_noise_shared); n = 2 points, M = 64 paths, K = 2 steps, one stream."""
import math

import pytest
import torch

import deeppicarditeration_amd as dpi
import net_weight_cases as T
from deeppicarditeration_amd import _lib as L
from deeppicarditeration_amd import data as D

pytestmark = pytest.mark.gpu
N, M = 2, 64
BOTH, PREPARED = L.DPI_BOTH, L.DPI_PREPARED
WITHOUT, DIFFER, NO_BASELINE = "without a dpi_label_prepare", "arguments differ", "no dpi_point_baseline"


@pytest.fixture(scope="module")
def setup():
    c = next(c for c in T.CASES if T.case_id(c) == "unit-gbm-ELU-2x32-nx7-auto")
    eq, oeq = T.equations(c)
    module, _ = T.network(c, eq, oeq, T.SCALES[T.net_id(c)])
    gen = dpi.OnlineDataGenerator(eq, module, 1, 1, device="cuda:0", t_always_uniform=True, n_estimate_terminal=M,
                                  n_estimate_integral=M, n_euler_steps=T.K, seed=T.SEED, epoch=T.EPOCH)
    tx, pb = gen.sample_t_and_x(N, point_base=0)
    return gen, tx, pb


def _workspace(gen, tx, paths=M):
    """A fresh workspace of the prepared size with the points' baseline on it."""
    ws = D.new_workspace(gen.workspace_bytes(N, paths, prepared=True), "cuda:0")
    gen.point_baseline(tx, ws=ws)
    return ws


def test_prepared_call_without_a_prepare(setup):
    gen, tx, pb = setup
    ws = _workspace(gen, tx)
    with pytest.raises(L.DPIError, match=WITHOUT):
        gen.label_moments(tx, pb, M, 0, M, BOTH | PREPARED, ws)


@pytest.mark.parametrize("what", ["seed", "point_base", "m_end", "flags"])
def test_prepared_call_that_differs_is_refused_and_consumes_the_record(setup, what):
    gen, tx, pb = setup
    paths = 2 * M if what == "m_end" else M  # m_end = 64 against M = 128
    ws = _workspace(gen, tx, paths)
    gen.label_prepare(tx, pb, paths, 0, paths, BOTH, ws)
    seed = gen.seed
    try:
        with pytest.raises(L.DPIError, match=DIFFER):
            if what == "seed":
                gen.seed = seed + 1
                gen.label_moments(tx, pb, paths, 0, paths, BOTH | PREPARED, ws)
            elif what == "point_base":
                gen.label_moments(tx, pb + 1, paths, 0, paths, BOTH | PREPARED, ws)
            elif what == "m_end":
                gen.label_moments(tx, pb, paths, 0, M, BOTH | PREPARED, ws)
            else:
                gen.label_moments(tx, pb, paths, 0, paths, L.DPI_TERMINAL | PREPARED, ws)
    finally:
        gen.seed = seed
    with pytest.raises(L.DPIError, match=WITHOUT):  # the refusal consumed the record
        gen.label_moments(tx, pb, paths, 0, paths, BOTH | PREPARED, ws)


def test_matching_prepared_call_is_the_plain_call_once(setup):
    gen, tx, pb = setup
    ws = _workspace(gen, tx)
    plain = gen.label_moments(tx, pb, M, 0, M, BOTH, ws)
    gen.label_prepare(tx, pb, M, 0, M, BOTH, ws)
    prepared = gen.label_moments(tx, pb, M, 0, M, BOTH | PREPARED, ws)
    with pytest.raises(L.DPIError, match=WITHOUT):
        gen.label_moments(tx, pb, M, 0, M, BOTH | PREPARED, ws)
    torch.cuda.synchronize()
    assert torch.isfinite(plain).all() and torch.equal(plain, prepared)


def test_unprepared_call_invalidates_the_prepare(setup):
    gen, tx, pb = setup
    ws = _workspace(gen, tx)
    gen.label_prepare(tx, pb, M, 0, M, BOTH, ws)
    gen.label_moments(tx, pb, M, 0, M, BOTH, ws)
    with pytest.raises(L.DPIError, match=WITHOUT):
        gen.label_moments(tx, pb, M, 0, M, BOTH | PREPARED, ws)
    torch.cuda.synchronize()


def test_forgotten_workspace_has_no_baseline(setup):
    gen, tx, pb = setup
    ws = _workspace(gen, tx)
    gen.label_moments(tx, pb, M, 0, M, BOTH, ws)
    L.check(gen.lib.dpi_workspace_forget(D._ptr(ws), ws.numel()), "dpi_workspace_forget")
    with pytest.raises(L.DPIError, match=NO_BASELINE):
        gen.label_moments(tx, pb, M, 0, M, BOTH, ws)
    torch.cuda.synchronize()


def test_refused_call_leaves_the_launch_timer_armed(setup):
    """A call refused behind its arguments (no baseline on the workspace) records nothing on the armed
    slot: dpi_launch_timer_ms answers DPI_ERR_ARG, and the next label call that launches records it."""
    gen, tx, pb = setup
    lib = gen.lib
    ws = D.new_workspace(gen.workspace_bytes(N, M, prepared=True), "cuda:0")
    ms = L.c_float(-1.0)
    L.check(lib.dpi_launch_timer_arm(0), "dpi_launch_timer_arm")
    with pytest.raises(L.DPIError, match=NO_BASELINE):
        gen.label_moments(tx, pb, M, 0, M, BOTH, ws)
    assert lib.dpi_launch_timer_ms(0, ms) == L.DPI_ERR_ARG
    assert "no launch recorded on this slot since it was armed" in L.last_error()
    gen.point_baseline(tx, ws=ws)
    gen.label_moments(tx, pb, M, 0, M, BOTH, ws)
    assert lib.dpi_launch_timer_ms(0, ms) == L.DPI_OK
    assert math.isfinite(ms.value) and ms.value >= 0.0
