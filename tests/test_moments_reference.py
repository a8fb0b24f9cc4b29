"""The fp64 reference of the label moments (oracle/dpi_oracle.py path_contributions, path_contributions_hess,
path_moments) for every case tests/test_gpu_moments.py runs on the GPU (tests/moments_cases.py) - no device
needed.

pin        mean(c) (+ g(x)) is labels_grad (labels_grad_hess, Hessian block included) of the same case to
           1e-12 (of max(1, the largest label)), and with one estimator alone its return_parts half: the
           per-path rows are the label's, TD, SDGD v = 7 and v = 100, M = 100 and M = 1 included.
yardstick  the fp64 rows rounded to fp32, squared and summed in fp32 in the device's order give both halves
           within 1e-6 of fp64 in the metrics e1, e2 of moments_cases: no case cancels catastrophically, so
           an fp32 kernel has 100 x of room under the GPU tests' 1e-4.  A condition on the inputs.
mutant     each fault of moments_cases.FAULTS moves sum c^2 by >= 1e-3 (10 x the GPU bar) on an entry it
           touches at every point of every case that reaches its edge, and by exactly 0.0 everywhere in the
           cases that cannot reach it (shown, not assumed).

Points: the oracle's own (sample_points; the device's agree to 2e-5).  Each reference's pieces are computed
once and shared by the three tests."""
import numpy as np
import pytest

import moments_cases as MC
import net_weight_cases as T
from oracle import dpi_oracle as O

PIN, YARDSTICK, MUTANT_FLOOR = 1e-12, 1e-6, 1e-3
REFS = MC.ref_cases()
_CACHE = {}


def _setup(mc):
    """(oeq, onet, tx, pieces per point) of a reference, once."""
    key = MC.ref_id(mc)
    if key not in _CACHE:
        _, oeq, _, onet = MC.build(mc)
        tx = O.sample_points(oeq, T.N, T.SEED, T.EPOCH, 0)
        _CACHE[key] = (oeq, onet, tx, [MC.pieces(mc, oeq, onet, tx[r], r) for r in range(T.N)])
    return _CACHE[key]


def _labels(mc, oeq, onet, tx):
    """(both, terminal part, integral part) of the oracle's label functions."""
    M = mc.c.M
    if mc.c.hess:
        return O.labels_grad_hess(oeq, onet, tx, M, T.K, T.SEED, T.EPOCH, 0, return_parts=True)
    return O.labels_grad(oeq, onet, tx, M, T.K, T.SEED, T.EPOCH, 0, v=mc.c.v, delta_t=MC.delta_t(mc), return_parts=True)


@pytest.mark.parametrize("mc", REFS, ids=MC.ref_id)
def test_per_path_rows_are_the_labels(mc):
    oeq, onet, tx, pcs = _setup(mc)
    M = mc.c.M
    ref = _labels(mc, oeq, onet, tx)[{MC.BOTH: 0, MC.TERMINAL: 1, MC.INTEGRAL: 2}[mc.flags]]
    rows = []
    for p in pcs:
        y = p.c[:M].mean(0)
        if mc.flags & MC.TERMINAL:
            y[0] += p.g
        rows.append(np.concatenate([y, p.h[:M].mean(0)]) if mc.c.hess else y)
    err = np.abs(np.stack(rows) - ref).max() / max(1.0, np.abs(ref).max())
    # path_moments, what the GPU tests compare with, sums the same rows
    S = MC.reference(mc, oeq, onet, tx)
    for r, p in enumerate(pcs):
        own = [p.c[:M].sum(0), (p.c[:M] ** 2).sum(0)] + ([p.h[:M].sum(0), (p.h[:M] ** 2).sum(0)] if mc.c.hess else [])
        for k, (a, b) in enumerate(zip(own, S[:4])):  # sums in their e1 scale (a batch's size moves BLAS's rounding)
            scale = np.sqrt(M * own[k + 1]) if k % 2 == 0 else a
            assert (np.abs(a - b[r]) <= 1e-12 * scale).all(), MC.ref_id(mc)
        assert S.g[r] == p.g
    print(MC.ref_id(mc), "pin", err)
    assert err <= PIN, err


def yardstick(mc):
    """Largest e1 / e2 (and, for Hessian labels, eh: the Hessian sums' e1) of the fp32 device-order sums."""
    oeq, onet, tx, _ = _setup(mc)
    ref = MC.reference(mc, oeq, onet, tx)
    assert (ref.S2 > 0).all(), "an entry of sum c^2 is zero: e1 and e2 have no scale there"
    assert ref.H2 is None or (ref.H2 > 0).all()
    return ref.yard


@pytest.mark.parametrize("mc", REFS, ids=MC.ref_id)
def test_fp32_in_device_order_is_within_1e6(mc):
    y = yardstick(mc)
    print(MC.ref_id(mc), "yardstick", {k: f"{v:.2e}" for k, v in y.items()})
    assert all(v <= YARDSTICK for v in y.values()), y


@pytest.mark.parametrize("mc", REFS, ids=MC.ref_id)
def test_every_fault_moves_the_second_half(mc):
    oeq, onet, tx, pcs = _setup(mc)
    nx, M = oeq.nx, mc.c.M
    base = [MC.restate(p) for p in pcs]
    for p, (S1, S2) in zip(pcs, base):  # the restatement without a fault is the oracle's own sums
        assert np.allclose(S1, p.c[:M].sum(0), rtol=0, atol=1e-12 * np.sqrt(M * S2).max())
        assert np.allclose(S2, (p.c[:M] ** 2).sum(0), rtol=1e-12, atol=0)
    effects, exempt = {}, []
    for fault in MC.FAULTS:
        cols = MC.touched(fault, nx)
        per_point, other = [], 0.0
        for p, (S1, S2) in zip(pcs, base):
            m1, m2 = MC.restate(p, fault)
            e = MC.e2(m2, S2)
            per_point.append(e[cols].max() if cols else 0.0)
            other = max(other, np.delete(e, cols).max() if len(cols) < len(e) else 0.0)
        assert other == 0.0, (fault, "moves a column it does not touch", other)
        if all(e == 0.0 for e in per_point):
            exempt.append(fault)  # this case cannot reach the fault's edge: shown, not assumed
            assert not MC.reached(fault, mc, nx), (fault, "is reached by this case and moves nothing")
        else:
            effects[fault] = min(per_point)
            assert MC.reached(fault, mc, nx), (fault, "moves a case that should not reach it", per_point)
    weakest = min(effects, key=effects.get)
    print(MC.ref_id(mc), "weakest", weakest, f"{effects[weakest]:.2e}", "exempt", exempt)
    weak = {k: v for k, v in effects.items() if v < MUTANT_FLOOR}
    assert not weak, ("faults that move sum c^2 by less than 1e-3 at some point", weak)
