"""The network phase of every label-kernel family against the fp64 oracle, with nets whose share of
the label makes the suite's bar bite (tests/net_weight.py, tests/net_weight_cases.py).

The other kernel-vs-oracle tests use nets at torch's default initialisation, where the network's term
(T - t) (f(u, grad u) - f_b) is 1e-5 .. 1e-2 of the label: a hidden unit lost at a tile tail, a wrong
column of W1, or (PISGradNet) the whole GEMM chain returning zero can stay under rel-L2 1e-4.  Here every
case first passes net_weight.gate on the CPU - the network carries 5 % .. 95 % of every block, and each
structural mutant of the net moves the oracle's label by >= 1e-3, 10 x the bar (the mutants in
tests/test_net_weight_gates.py, the share band here again at the device's points) - and then one label
call is compared with the gate's reference: rel-L2 < 1e-4 per block (value, gradient, Hessian), all labels
finite, no warning inside the call, and range_status() == 0 after it (a SplitRangeWarning would mean the
"auto" case silently ran in fp32).

Cases (net_weight_cases.CASES): all 20 rows of the unit table with [16] and [32, 32] (nx = 7, 129 on the
wide rows, TD at dt = 0.3, GBM with the full Hessian diagonal); the specialised width classes at their
edges ([64, 64] at nx 1, 7, 80, 96, 113, 128; the three workload nets at nx = 100, GBM with SDGD v = 100
and v = 7; M = 100 with partial blocks); Hessian labels; the general family and the gradient heads;
PISGradNet [512] * L for L = 1..4 and [32, 32], DPI_PIS_FUSED=0 once, TD once (3 x 128 = 384 chain rows
plus the 3 baseline rows: the partial 64-row tile runs).  n = 3, M = 128, K = 2, seed 1, epoch 1."""
import warnings

import numpy as np
import pytest

import deeppicarditeration_amd as dpi
import net_weight as NW
import net_weight_cases as T
from deeppicarditeration_amd import _lib as L
from oracle import dpi_oracle as O

pytestmark = pytest.mark.gpu
TOL = 1e-4


def _generator(c, eq, module):
    return dpi.OnlineDataGenerator(eq, module, 1, 1, device="cuda:0", t_always_uniform=True, n_estimate_terminal=c.M,
                                   n_estimate_integral=c.M, n_euler_steps=T.K, seed=T.SEED, epoch=T.EPOCH,
                                   estimate_delta_t=T.DT if c.variant == "td" else None,
                                   hessian_approximation={"method": "SDGD", "kwargs": {"v": c.v}} if c.v else None,
                                   partial_blocks=True if c.M % L.DPI_PATH_BLOCK else None)


@pytest.mark.parametrize("case", T.CASES, ids=T.case_id)
def test_network_phase_vs_oracle(case, monkeypatch):
    c = case
    eq, oeq = T.equations(c)
    module, onet = T.network(c, eq, oeq)
    if c.fused is not None:  # read per call
        monkeypatch.setenv("DPI_PIS_FUSED", c.fused)
    lib = L.load()
    L.check(lib.dpi_set_gemm_precision(L.DPI_GEMM_F32 if c.mode == "f32" else L.DPI_GEMM_AUTO), "gemm precision")
    try:
        gen = _generator(c, eq, module)
        general = c.group in ("general", "head")
        assert gen.net.family(gen.problem, c.variant == "td") == (L.DPI_FAMILY_GENERAL if general else
                                                                 L.DPI_FAMILY_SPECIALISED)
        assert not c.head or gen.net.desc.endswith("-" + c.head)
        assert not c.pis or gen.net.desc.startswith("pisgrad")
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            if c.variant == "fb":  # points and labels in one call: one launch where the fused baseline fits
                tx, y = gen.sample_with_gradients(T.N)
            else:
                tx, pb = gen.sample_t_and_x(T.N, point_base=0)
                y = (gen.generate_with_gradients_and_hessians(tx, point_base=pb) if c.hess else
                     gen.generate_with_gradients(tx, point_base=pb))
        status = gen.range_status()
        y = y.cpu().numpy()
    finally:
        L.check(lib.dpi_set_gemm_precision(L.DPI_GEMM_AUTO), "gemm precision")
    txh = tx.cpu().double().numpy()
    assert np.allclose(txh, O.sample_points(oeq, T.N, T.SEED, T.EPOCH, 0), rtol=0, atol=2e-5)
    if c.variant == "td":
        assert (txh[:, 0] + T.DT < 1).any() and (txh[:, 0] + T.DT >= 1).any()  # t = 0.81, 0.06, 0.18
    info = {}
    # share band and finiteness at the device's own points; the mutant gate is tests/test_net_weight_gates.py's
    ref = T.reference(c, oeq, onet, txh, info, with_mutants=False)
    parts = NW.blocks(y, ref, c.nx if c.hess else None)
    print(T.case_id(c), "scales", T.scales(c), "share", {k: round(v, 3) for k, v in info["share"].items()}, "rel-L2", parts)
    assert y.shape == ref.shape and np.isfinite(y).all()
    assert status == 0
    assert all(p < TOL for p in parts.values()), parts
