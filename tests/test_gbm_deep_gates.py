"""Every net of tests/gbm_deep_cases.py passes tests/net_weight.py's gate on the CPU with the fp64 oracle
alone, at the oracle's points: the network's share of the label lies in [0.05, 0.95] on the value column
and on the gradient block, and every structural mutant moves the label by >= 1e-3 rel-L2 on some block,
or by exactly 0.0 on both (out_bias: GBM's f does not read u).  These are conditions on the inputs of
tests/test_gpu_gbm_deep.py, not tolerances on the kernel; no device is needed."""
import math

import pytest

import gbm_deep_cases as G
from oracle import dpi_oracle as O

NETS = list({G.net_id(c): c for c in G.CASES}.values())


def test_the_table():
    ids = [G.case_id(c) for c in G.CASES]
    assert len(ids) == len(set(ids))
    assert set(G.SCALES) == {G.net_id(c) for c in G.CASES}
    for h, o, _ in G.SCALES.values():
        assert all(s > 0 and math.log2(s).is_integer() for s in (h, o)), (h, o)
    # what the table has to cover: both activations, SDGD (v = nx = 7 among them) and the exact diagonal,
    # the three width classes, L = 1 and L = 8, the widest layer not first, nx = 100 and nx = 128
    assert {c.act for c in G.CASES} == {"ELU", "Tanh"}
    assert {0, 7, 100} <= {c.v for c in G.CASES} and any(c.v == c.nx == 7 for c in G.CASES)
    assert {16, 32, 64} <= {max(c.widths) for c in G.CASES}
    assert {1, 8} <= {len(c.widths) for c in G.CASES}
    assert any(max(c.widths) != c.widths[0] for c in G.CASES)
    assert {100, 128} <= {c.nx for c in G.CASES}
    assert all(c.eq == "gbm" and max(c.widths) <= 64 and len(c.widths) <= 8 for c in G.CASES)


@pytest.mark.parametrize("case", NETS, ids=G.net_id)
def test_case_passes_the_gate(case):
    eq, oeq = G.equations(case)
    _, onet = G.network(case, eq, oeq)
    info = {}
    ref = G.reference(case, oeq, onet, O.sample_points(oeq, G.N, G.SEED, G.EPOCH, 0), info)
    weakest = min((max(e.values()), n) for n, e in info["mutants"].items() if n not in info["exempt"])
    print(G.net_id(case), G.scales(case), "share", info["share"], "weakest mutant", weakest, "exempt", info["exempt"])
    assert ref.shape == (G.N, 1 + case.nx)
    assert set(info["exempt"]) <= {"out_bias"}
