"""Reference pin of the gradient-head labels (NETWORK.TYPE ValueGradient / OnlyGradient): the fp64
oracle, given a net whose value_grad answers from the head's output columns (tests/heads_util.py
HeadNet), reproduces the reference's sample_with_gradients labels of tests/golden/heads/*.npz (made
by tests/golden/make_golden_heads.py) at the project's pin bar, rel-L2 <= 1e-12 on the value column
and on the gradient block.  CPU, fp64."""
import numpy as np
import pytest

import golden_util as G
import heads_util as H
from oracle import dpi_oracle as O

PIN = 1e-12


def test_fixture_set():
    """Cha and OU at nx = 100 with both heads and both activations, and an nx = 7 case."""
    seen = {(str(f["eq"]), str(f["head"]), str(f["acts"][0]), int(f["eqkw_nx"])) for f in map(H.load, H.HEAD_CASES)}
    for eq in ("Cha", "OUProcessEquation"):
        for head in ("ValueGradient", "OnlyGradient"):
            for act in ("ELU", "Tanh"):
                assert (eq, head, act, 100) in seen, (eq, head, act)
    assert any(nx == 7 for *_, nx in seen)


@pytest.mark.parametrize("name", H.HEAD_CASES)
def test_oracle_reproduces_reference_head_labels(name):
    f = H.load(name)
    eq = G.oracle_equation(f)
    net = H.fixture_net(f)
    n_out = net.W[-1].shape[0]
    assert n_out == {"ValueGradient": 1 + eq.nx, "OnlyGradient": eq.nx}[str(f["head"])]
    y = O.labels_grad(eq, net, f["tx"], int(f["M"]), int(f["K"]), int(f["seed"]), int(f["epoch"]), int(f["point_base"]))
    parts = O.rel_l2_parts(y, f["y"])
    print(name, parts)
    assert parts["value"] <= PIN and parts["grad"] <= PIN, parts
    # the head matters: the zero net's labels are not these
    zero = O.rel_l2_parts(O.labels_grad(eq, O.ZeroNet(), f["tx"], int(f["M"]), int(f["K"]), int(f["seed"]),
                                        int(f["epoch"]), int(f["point_base"])), f["y"])
    assert zero["grad"] > 1e-6 or zero["value"] > 1e-6, zero
    assert np.isfinite(y).all()
