"""Reference pin of the terminal-enforcing labels (NETWORK.cls PicardSolutionEnforceTerminal): the fp64
oracle, given the twin of the wrapper (tests/terminal_util.py TerminalNet: u = g + (T - t) N, or
g_x + (T - t) N read as u_x with u = 0), reproduces the reference's own sample_with_gradients labels of
tests/golden/terminal/*.npz (made by tests/golden/make_golden_terminal.py from the reference's class) at
the project's pin bar, rel-L2 <= 1e-12 on the value column and on the gradient block.  CPU, fp64."""
import numpy as np
import pytest

import golden_util as G
import terminal_util as T
from oracle import dpi_oracle as O

PIN = 1e-12


def _labels(f, eq, net):
    return O.labels_grad(eq, net, f["tx"], int(f["M"]), int(f["K"]), int(f["seed"]), int(f["epoch"]), int(f["point_base"]))


def test_fixture_set():
    """Cha and OU at nx = 100 with both types and both activations, and two nx = 7 cases; every one made
    from the reference's own class."""
    fs = [T.load(c) for c in T.TERMINAL_CASES]
    seen = {(str(f["eq"]), str(f["type"]), str(f["acts"][0]), int(f["eqkw_nx"])) for f in fs}
    for eq in ("Cha", "OUProcessEquation"):
        for typ in ("Value", "OnlyGradient"):
            for act in ("ELU", "Tanh"):
                assert (eq, typ, act, 100) in seen, (eq, typ, act)
    assert sum(nx == 7 for *_, nx in seen) >= 2
    assert {str(f["cls"]) for f in fs} == {"PicardSolutionEnforceTerminal"}
    assert {int(f["K"]) for f in fs} == {1, 2}


@pytest.mark.parametrize("name", T.TERMINAL_CASES)
def test_oracle_reproduces_reference_terminal_labels(name):
    f = T.load(name)
    eq = G.oracle_equation(f)
    net = T.fixture_net(f, eq)
    assert net.inner.W[-1].shape[0] == {"Value": 1, "OnlyGradient": eq.nx}[str(f["type"])]
    y = _labels(f, eq, net)
    parts = O.rel_l2_parts(y, f["y"])
    print(name, parts)
    assert np.isfinite(y).all()
    assert parts["value"] <= PIN and parts["grad"] <= PIN, parts
    # the ansatz matters: the bare inner network's labels are not these
    bare = O.rel_l2_parts(_labels(f, eq, net.inner), f["y"])
    print(name, "bare N", bare)
    assert max(bare["value"], bare["grad"]) > 1e-6, bare
