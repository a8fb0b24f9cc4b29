"""The numpy fp64 restatement of the PISGradNet core's four passes and of the objective around them
(tests/pis_fit_reference.py) against torch fp64 autograd of the existing objectives on
the whole PISGradNet, on every case of the GPU table, and the gates that show the yardstick sees each
structural error on every gradient case.  CPU only."""
import numpy as np
import pytest

import pis_fit_reference as R


@pytest.mark.parametrize("k", range(len(R.CASES)), ids=R.IDS)
def test_four_passes_equal_torch_fp64_autograd(k):
    """The loss and every parameter gradient of the PISGradNet (time networks included) to fp64 rounding,
    rtol 1e-12; a tensor whose fp64 gradient is exactly zero is compared absolutely, against 1e-12 x the
    largest gradient norm of the case."""
    loss, got = R.restated(k)
    want_loss, want = R.torch_fp64(k)
    assert len(got) == len(want) == len(R.param_names(R.CASES[k]))
    assert abs(loss - want_loss) <= 1e-12 * abs(want_loss)
    errs = R.tensor_errors(got, want)
    assert max(errs) <= 1e-12, dict(zip(R.param_names(R.CASES[k]), errs))


GRADIENT_CASES = [k for k, c in enumerate(R.CASES) if c[6] > 1e-9]


@pytest.mark.parametrize("k", GRADIENT_CASES, ids=[R.IDS[k] for k in GRADIENT_CASES])
def test_gates(k):
    """Each structural mutant moves the gradient by >= 1e-3 (10 x the parity bar of the GPU test) in the
    GPU test's own measure, the largest per-tensor rel-L2: pass 3 dropped, the N term of q dropped,
    v lambdabar_L^T dropped, taubar zeroed (seen in t_encoder's gradient) and one hidden unit zeroed."""
    _, full = R.restated(k)
    names = R.param_names(R.CASES[k])
    for mutant in R.MUTANTS:
        _, got = R.restated(k, mutant=mutant)
        errs = dict(zip(names, R.tensor_errors(got, full)))
        if mutant == "no_dtau":  # only tau's consumers see it
            errs = {n: e for n, e in errs.items() if n.startswith("t_encoder.") or n == "timestep_phase"}
            assert all(e == 0.0 for n, e in dict(zip(names, R.tensor_errors(got, full))).items()
                       if n.startswith("nn_module."))
        assert max(errs.values()) >= 1e-3, (mutant, errs)
    _, got = R.restated(k, zero_unit=True)
    assert R.worst_rel_l2(got, full) >= 1e-3


def test_value_kind_forms_no_q():
    """c <= 1e-9: only sp is formed and passes 2 and 3 are skipped."""
    k = next(k for k, c in enumerate(R.CASES) if c[6] <= 1e-9)
    case = R.CASES[k]
    net = R.make_net(case)
    tx = R.make_batch(k)[0].double()
    ps = [p.detach().numpy() for p in net.nn_module.parameters()]
    tau = np.zeros((case[0], R.NT))
    sp, q, st = R.core_forward(ps[0::2], ps[1::2], tau, tx[:, 1:].numpy(), grad=False)
    assert q is None and "lam" not in st and sp.shape == (case[0], 1)


def test_clip_cases_take_both_branches():
    import torch
    for k, case in enumerate(R.CASES):
        if not case[5]:
            continue
        tx, y, clip = R.make_batch(k)
        u, u_tx = R.fit._u_and_grad(R.make_net(case), tx.double())
        res = [u.detach() - y[:, :1].double()]
        if case[6] > 1e-9:
            res.append(u_tx.detach()[:, 1:] - y[:, 1:1 + case[1]].double())
        beyond = float((torch.cat(res, 1).abs() >= clip).double().mean())
        assert 0.1 <= beyond <= 0.9, (k, beyond)


def test_table_covers_the_axes():
    assert {c[0] for c in R.CASES} == {1, 64, 65, 100, 512}
    assert {c[1] for c in R.CASES} == {3, 10, 100, 128}
    assert {tuple(c[2]) for c in R.CASES} == {(16,), (64,) * 4, (130, 70), (512,) * 2, (512,) * 4}
    assert [c[0] for c in R.CASES if tuple(c[2]) == (512,) * 4] == [64]
    assert sorted(c[3] for c in R.CASES if c[3] != 1.0) == [0.5]
    assert {c[5] for c in R.CASES} == {False, True} and {c[6] for c in R.CASES} == {1.0, 0.1, 0.0}
