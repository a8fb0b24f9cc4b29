"""Every net of tests/net_weight_cases.py passes tests/net_weight.py's gate, on the CPU with the fp64
oracle alone: the share of the network in the label lies in [0.05, 0.95] on every block, every
structural mutant moves the label by >= 1e-3 rel-L2 on some block (or by exactly 0.0 on all of them, where
the equation cannot observe it), and the labels are finite.  This is what makes the rel-L2 < 1e-4 of
tests/test_gpu_network_phase.py a statement about the kernels' network phases; it needs no device.

Points: O.sample_points at the GPU tests' seed and epoch (the device draws the same points in fp32).
The share and mutant figures printed here (-s) are CPU-oracle figures, not device measurements."""
import math

import numpy as np
import pytest
import torch

import net_weight as NW
import net_weight_cases as T
from oracle import dpi_oracle as O

NETS = list({T.net_id(c): c for c in T.CASES}.values())


def _points(oeq):
    return O.sample_points(oeq, T.N, T.SEED, T.EPOCH, 0)


def test_the_table():
    from test_gpu_dispatch_rows import ROWS
    ids = [T.case_id(c) for c in T.CASES]
    assert len(ids) == len(set(ids))
    assert {(c.eq, c.act, c.variant) for c in T.CASES if c.group == "unit"} == set(ROWS) and len(ROWS) == 20
    assert set(T.SCALES) == {T.net_id(c) for c in T.CASES}
    for h, o, *_ in T.SCALES.values():
        assert all(s > 0 and math.log2(s).is_integer() for s in (h, o)), (h, o)


@pytest.mark.parametrize("case", NETS, ids=T.net_id)
def test_case_passes_the_gate(case):
    eq, oeq = T.equations(case)
    _, onet = T.network(case, eq, oeq)
    info = {}
    ref = T.reference(case, oeq, onet, _points(oeq), info)
    weakest = min((max(e.values()), n) for n, e in info["mutants"].items() if n not in info["exempt"])
    print(T.net_id(case), T.scales(case), "share", info["share"], "weakest mutant", weakest, "exempt", info["exempt"],
          f"max |label| {info['max_label']:.2e}")
    assert ref.shape == (T.N, 1 + case.nx + (case.nx ** 2 if case.hess else 0))


def test_exempt_mutants_are_exactly_invisible():
    """OU's f does not read u: without TD the output bias moves no label at all, bit for bit; with TD the
    terminal term reads u(t + dt, X), and the same mutant counts."""
    plain = next(c for c in NETS if c.group == "unit" and c.eq == "ou" and c.variant == "plain" and len(c.widths) == 2)
    td = plain._replace(variant="td")
    for c, exempt in ((plain, True), (td, False)):
        eq, oeq = T.equations(c)
        _, onet = T.network(c, eq, oeq)
        info = {}
        T.reference(c, oeq, onet, _points(oeq), info)
        assert ("out_bias" in info["exempt"]) == exempt
        assert all(x == 0.0 for x in info["mutants"]["out_bias"].values()) == exempt


# ------------------------------------------------------ why the table is needed: three nets that fail the band
def _gate(c, onet, oeq):
    return NW.gate(oeq, onet, _points(oeq), **T.oracle_kw(c))


def test_default_burgers_4x128_fails_the_share_band():
    c = next(c for c in NETS if c.group == "edge" and c.eq == "cha" and c.widths == (128,) * 4 and c.M == 128)
    eq, oeq = T.equations(c)
    _, onet = T.network(c, eq, oeq, (1, 1))
    with pytest.raises(AssertionError, match="share of the network"):
        _gate(c, onet, oeq)
    sh = NW.share(oeq, onet, _points(oeq), **T.oracle_kw(c))
    assert max(sh.values()) < 0.05, sh


def test_default_pisgradnet_4x512_fails_the_share_band():
    c = next(c for c in NETS if c.pis and c.widths == (512,) * 4 and c.variant == "plain")
    eq, oeq = T.equations(c)
    _, onet = T.network(c, eq, oeq, (1, 1))
    with pytest.raises(AssertionError, match="share of the network"):
        _gate(c, onet, oeq)
    sh = NW.share(oeq, onet, _points(oeq), **T.oracle_kw(c))
    assert max(sh.values()) < 0.05, sh


def test_every_parameter_x32_fails_the_share_band():
    """tests/test_gpu_range.py's net: every parameter x 32.  The label is the network's alone (and every
    ELU sits on a linear branch): share > 0.95."""
    c = next(c for c in NETS if c.group == "edge" and c.eq == "cha" and c.widths == (128,) * 4 and c.M == 128)
    eq, oeq = T.equations(c)
    module = T.default_module(c, eq)
    with torch.no_grad():
        for p in module.parameters():
            p.mul_(32.0)
    onet = NW.oracle_twin(module)
    with pytest.raises(AssertionError, match="share of the network"):
        _gate(c, onet, oeq)
    sh = NW.share(oeq, onet, _points(oeq), **T.oracle_kw(c))
    assert min(sh.values()) > 0.95 and np.isfinite(list(sh.values())).all(), sh
