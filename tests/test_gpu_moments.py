"""Both halves of `moments` (sum of c, sum of c^2 over the Monte-Carlo paths) of every label entry point
against the fp64 oracle, entry by entry (oracle/dpi_oracle.py path_moments; tests/moments_cases.py).

The first half divided by M is the label, compared with the oracle in the parity tests as a block norm.  The
second half is what sharding.py gathers and what the statistical known-answer test of tests/test_gpu_train.py
turns into its standard errors; it has arithmetic and stores of its own in paths_body's phase 3 (the
56-column form, the eighth dim-block, the wide instances' groups of seven), in the value column's c0 * c0
with its dead-lane selects and the per-lane GBM baseline, in PISGradNet's row finish and in every reducer.
A square formed after a lane reduction, the two estimators squared apart, a dead lane's baseline counted, a
sum and a square exchanged at d >= 112 or a block dropped from the second half's tree would leave every
label as it is.

For every point i and column j of one label call per case, with S1, S2 the fp64 reference over the M paths
the call summed:
    e1 = |S1_hip - S1| / sqrt(M S2)      e2 = |S2_hip - S2| / S2
every entry of both is below 1e-4, the project's parity tolerance applied entrywise in the entry's own scale
(Hessian labels: the Hessian sums too, in the scale sqrt(M sum h^2)); all moments are finite, no warning
inside the call, range_status() == 0, and a finalized call's label is moments[:, 0] / M (+ g(x)): bitwise
dpi_label_finalize of the returned moments, bitwise fp32 moments * (1 / M) on the gradient columns, within one
ulp of it plus g on the value column.  The ranged, prepared and reduced forms are also bitwise the single call.

tests/test_moments_reference.py holds, without a GPU: the reference pinned to labels_grad at 1e-12, the CPU
yardstick (the same rows in fp32 in the device's order: <= 1.7e-7 in e1 and e2 on every case) and the mutant
gate (each of the faults above moves sum c^2 by >= 3.2e-3 where a case reaches it).  Each case prints its
largest e1 and e2 and their ratio to the yardstick at its own points; the device's normals differ from libm's
by up to 2e-5, so ratios above 1 are expected.  They are reported, not asserted.

Measured on one MI355X (profiles/label_moments/test_gpu_moments.txt; per family in DESIGN.md §0), largest
e1 / e2 and their ratio to the yardstick:
    M = 128, 100 and 4160, every MLP kernel family         6.6e-7 / 3.5e-6     22 x / 29 x
    PISGradNet                                             1.8e-6 / 8.7e-6     51 x / 62 x
    M = 1 (one path's c and c^2)                           1.4e-5 / 2.8e-5     252 x / 213 x
    Hessian sums (scale sqrt(M sum h^2))                   2.5e-6              84 x
No case failed."""
import warnings

import numpy as np
import pytest
import torch

import deeppicarditeration_amd as dpi
import moments_cases as MC
import net_weight_cases as T
from deeppicarditeration_amd import _lib as L
from deeppicarditeration_amd import data as D
from oracle import dpi_oracle as O

pytestmark = pytest.mark.gpu
TOL = 1e-4
INF = float("inf")


def _generator(mc, eq, module):
    c = mc.c
    return dpi.OnlineDataGenerator(eq, module, 1, 1, device="cuda:0", t_always_uniform=True, n_estimate_terminal=c.M,
                                   n_estimate_integral=c.M, n_euler_steps=T.K, seed=T.SEED, epoch=T.EPOCH,
                                   estimate_delta_t=T.DT if c.variant == "td" else None,
                                   hessian_approximation={"method": "SDGD", "kwargs": {"v": c.v}} if c.v else None,
                                   partial_blocks=True if c.M % L.DPI_PATH_BLOCK else None)


def _call(mc, gen):
    """One label call through the case's entry point: (tx, ws, y or None, moments, Hessian sums or None,
    [(m_begin, m_end, moments of that range)] for the ranged form)."""
    M, flags, entry = mc.c.M, mc.flags, mc.entry
    if entry == "sample":  # dpi_sample_with_gradients: the one-launch hand-off where it fits
        tx, y = gen.sample_with_gradients(T.N)
        return tx, gen._workspace(T.N, M), y, gen.last_moments, None, []
    tx, pb = gen.sample_t_and_x(T.N, point_base=0)
    if entry == "generate":  # dpi_generate_with_gradients
        y = gen.generate_with_gradients(tx, point_base=pb)
        return tx, gen._workspace(T.N, M), y, gen.last_moments, None, []
    if entry == "hess":  # dpi_label_moments_hessians
        ws = gen.point_baseline(tx, hessians=True)
        mom, hs = gen.label_moments_hessians(tx, pb, M, 0, M, ws, flags)
        return tx, ws, None, mom, hs, []
    if entry == "prepared":  # dpi_label_prepare + DPI_PREPARED, bitwise the unprepared call
        ws = D.new_workspace(gen.workspace_bytes(T.N, M, prepared=True), "cuda:0")
        gen.point_baseline(tx, ws=ws)
        plain = gen.label_moments(tx, pb, M, 0, M, flags, ws)
        gen.label_prepare(tx, pb, M, 0, M, flags, ws)
        mom = gen.label_moments(tx, pb, M, 0, M, flags | L.DPI_PREPARED, ws)
        assert torch.equal(mom, plain)
        return tx, ws, None, mom, None, []
    ws = gen.point_baseline(tx)
    if entry == "finalize":  # dpi_label_moments_finalize
        y, mom = gen.label_moments_finalize(tx, pb, M, flags, ws, bound=INF)
        return tx, ws, y, mom, None, []
    if entry == "moments":  # dpi_label_moments
        return tx, ws, None, gen.label_moments(tx, pb, M, 0, M, flags, ws), None, []
    assert entry == "ranges" and M == 2 * MC.BLOCK  # two ranges through dpi_moments_reduce, bitwise the single call
    single = gen.label_moments(tx, pb, M, 0, M, flags, ws)
    parts = [(a, a + MC.BLOCK, gen.label_moments(tx, pb, M, a, a + MC.BLOCK, flags, ws)) for a in (0, MC.BLOCK)]
    mom = gen.moments_reduce(torch.stack([p[2] for p in parts]))
    assert torch.equal(mom, single)
    return tx, ws, None, mom, None, parts


def _errors(mom, ref, M):
    mom = np.asarray(mom, np.float64)
    return MC.e1(mom[:, 0], ref.S1, ref.S2, M), MC.e2(mom[:, 1], ref.S2)


@pytest.mark.parametrize("mc", MC.CASES, ids=lambda mc: mc.name)
def test_moments_vs_oracle(mc, monkeypatch):
    c, M = mc.c, mc.c.M
    eq, oeq, module, onet = MC.build(mc)
    lib = L.load()
    L.check(lib.dpi_set_gemm_precision(L.DPI_GEMM_F32 if c.mode == "f32" else L.DPI_GEMM_AUTO), "gemm precision")
    try:
        with warnings.catch_warnings():  # M = 1: the constructor's note that one path costs what 64 cost
            warnings.simplefilter("ignore", D.PartialBlockNote)
            gen = _generator(mc, eq, module)
        general = c.group in ("general", "head")
        assert gen.net.family(gen.problem, c.variant == "td") == (L.DPI_FAMILY_GENERAL if general else
                                                                 L.DPI_FAMILY_SPECIALISED)
        assert not c.pis or gen.net.desc.startswith("pisgrad")
        assert not mc.terminal or gen.net.desc.endswith("-terminal")
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            tx, ws, y, mom, hs, parts = _call(mc, gen)
        status = gen.range_status()
        if y is not None:  # what dpi_label_finalize makes of these moments, and g(x) alone
            y_lib = gen.finalize(mom, M, mc.flags, ws, bound=INF).cpu().numpy()
            gx = gen.finalize(torch.zeros_like(mom), M, mc.flags, ws, bound=INF).cpu().numpy()[:, 0]
            y = y.cpu().numpy()
        mom = mom.cpu().numpy()
        hs = None if hs is None else hs.cpu().numpy()
        parts = [(a, b, p.cpu().numpy()) for a, b, p in parts]
    finally:
        L.check(lib.dpi_set_gemm_precision(L.DPI_GEMM_AUTO), "gemm precision")
    txh = tx.cpu().double().numpy()
    assert np.allclose(txh, O.sample_points(oeq, T.N, T.SEED, T.EPOCH, 0), rtol=0, atol=2e-5)
    assert mom.shape == (T.N, 2, 1 + c.nx) and mom.dtype == np.float32
    assert np.isfinite(mom).all() and (hs is None or np.isfinite(hs).all())
    assert status == 0

    ref = MC.reference(mc, oeq, onet, txh)
    a1, a2 = _errors(mom, ref, M)
    worst = {"e1": a1.max(), "e2": a2.max()}
    if hs is not None:
        assert hs.shape == ref.H1.shape
        worst["eh"] = MC.e1(hs, ref.H1, ref.H2, M).max()
    for a, b, p in parts:  # each range against its own paths
        r = MC.reference(mc, oeq, onet, txh, a, b)
        for k, e in zip(("e1", "e2"), _errors(p, r, b - a)):
            worst[k] = max(worst[k], e.max())
    print(mc.name, "worst", {k: f"{v:.2e}" for k, v in worst.items()},
          "yardstick", {k: f"{v:.2e}" for k, v in ref.yard.items()},
          "ratio", {k: f"{worst[k] / ref.yard[k]:.1f}" for k in worst})

    if y is not None:
        assert np.array_equal(y, y_lib)
        lab = mom[:, 0] * (np.float32(1.0) / np.float32(M))
        assert lab.dtype == np.float32 and np.array_equal(y[:, 1:], lab[:, 1:])
        v = lab[:, 0].astype(np.float64) + (gx if mc.flags & MC.TERMINAL else 0.0)
        assert (np.abs(y[:, 0] - v) <= np.spacing(np.abs(v).astype(np.float32))).all()
    assert all(v < TOL for v in worst.values()), worst
    assert (a1 < TOL).all() and (a2 < TOL).all()
