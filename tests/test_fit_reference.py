"""The numpy fp64 restatement of the device fit's five passes (tests/fit_reference.py)
against the existing torch objectives under fp64 autograd, on every case of the GPU table, and the gates
that show the yardstick can see a structural error on each of them.  CPU only."""
import numpy as np
import pytest
import torch

import fit_reference as R


def _params(k):
    net = R.make_net(R.CASES[k])
    ps = [p.detach().numpy() for p in net.parameters()]
    return ps[0::2], ps[1::2]


def _run(k, **kw):
    case = R.CASES[k]
    tx, y, clip = R.make_batch(k)
    Ws, bs = _params(k)
    return R.reference(Ws, bs, case[3], tx.numpy(), y.numpy(), case[4], clip, case[6], **kw)


def _flat(dWs, dbs):
    return np.concatenate([g.ravel() for pair in zip(dWs, dbs) for g in pair])


@pytest.mark.parametrize("k", range(len(R.CASES)), ids=R.IDS)
def test_five_passes_equal_torch_fp64_autograd(k):
    """Every loss and every parameter gradient, to fp64 rounding: rtol 1e-12 (the bar of
    tests/test_fit_golden.py), with elements that cancel to nothing measured against their tensor's
    largest entry."""
    losses, dWs, dbs = _run(k)
    want_losses, want = R.torch_fp64(k)
    np.testing.assert_allclose(losses, want_losses, rtol=1e-12, atol=0)
    got = [g for pair in zip(dWs, dbs) for g in pair]
    assert len(got) == len(want)
    for g, w in zip(got, want):
        np.testing.assert_allclose(g.reshape(w.shape), w, rtol=1e-12, atol=1e-12 * np.abs(w).max())


@pytest.mark.parametrize("k", range(len(R.CASES)), ids=R.IDS)
def test_gates(k):
    """A structural error moves the yardstick far beyond the parity bars: dropping pass 4 (the term
    torch's create_graph produces; gradient kinds, the value kind has no pass 4) by >= 1e-2, zeroing the
    last unit of the last hidden layer by >= 1e-3, and the clip cases take both branches of rho."""
    case = R.CASES[k]
    B, nx, widths, act, beta, clipped, c, extra = case
    _, dWs, dbs = _run(k)
    full = _flat(dWs, dbs)
    if c > 1e-9:
        _, dW4, db4 = _run(k, drop_tangent=True)
        assert R.rel_l2(_flat(dW4, db4), full) >= 1e-2
    tx, y, clip = R.make_batch(k)
    Ws, bs = _params(k)
    Ws, bs = [W.copy() for W in Ws], [b.copy() for b in bs]
    Ws[-2][-1, :] = 0.0
    bs[-2][-1] = 0.0
    _, dWz, dbz = R.reference(Ws, bs, act, tx.numpy(), y.numpy(), beta, clip, c)
    assert R.rel_l2(_flat(dWz, dbz), full) >= 1e-3
    if clipped:
        net = R.make_net(case)
        u, u_tx = R.fit._u_and_grad(net, tx.double())
        res = [u.detach() - y[:, :1].double()]
        if c > 1e-9:
            res.append(u_tx.detach()[:, 1:] - y[:, 1:1 + nx].double())
        beyond = float((torch.cat(res, 1).abs() >= clip).double().mean())
        assert 0.1 <= beyond <= 0.9, beyond


def test_table_covers_the_axes():
    B = {c[0] for c in R.CASES}
    assert B == {1, 64, 65, 100, 512}
    assert {c[1] for c in R.CASES} == {7, 100, 128, 256}
    assert {tuple(c[2]) for c in R.CASES} == {(16,), (32, 32), (128,) * 4, (24,) * 8, (65, 65), (129,), (256,) * 8}
    assert {c[3] for c in R.CASES} == {"ELU", "Tanh"} and {c[4] for c in R.CASES} == {0.0, 0.7}
    assert {c[5] for c in R.CASES} == {False, True} and {c[6] for c in R.CASES} == {1.0, 0.1, 0.0}
    assert sum(1 for c in R.CASES if c[7] == c[1] ** 2) == 1
