"""The outer fit of a terminal-enforcing solution (NETWORK.cls PicardSolutionEnforceTerminal) against the
reference's own training steps on its own class (tests/golden/fit_terminal/*.npz, made by
tests/golden/make_fit_golden_terminal.py from picard/solution_jac.py:167-213 around
picard/solution_enforce_terminal.py:9-27): same initial weights, same batches, same optimizer -> the
per-step losses agree to rtol 1e-12 and the final weights to fp64 rounding, the bars of
tests/test_fit_golden.py.  The objectives are fit.py's, computed on this build's wrapper module.
CPU, fp64."""
import json
from pathlib import Path

import numpy as np
import pytest
import torch

from deeppicarditeration_amd import equations as eqs
from deeppicarditeration_amd import fit as F
from deeppicarditeration_amd.solution import PicardSolutionEnforceTerminal, construct_mlp

DIR = Path(__file__).parent / "golden" / "fit_terminal"
CASES = sorted(p.stem for p in DIR.glob("fit_*.npz"))


def _load(name):
    with np.load(DIR / f"{name}.npz", allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def _train_cfg(cfg):
    scaler = cfg["scaler"]
    return {"LOSS": {"beta": cfg["beta"],
                     "SCALER": {"cls": scaler[0] if scaler else None, "kwargs": scaler[1] if scaler else {}},
                     "FN": {"cls": "LossFnLinearClip" if cfg["clip"] is not None else None,
                            "kwargs": {"clip": cfg["clip"]}},
                     "use_aux_loss": False, "weight_aux_loss": 0.1},
            "NUM_HESS_SAMPLES": -1, "OPTIMIZER": {"cls": "Adam", "kwargs": {"lr": cfg["lr"]}}}


def test_fixture_set():
    cfgs = [json.loads(str(_load(c)["cfg"])) for c in CASES]
    assert {c["type"] for c in cfgs} == {"Value", "OnlyGradient"}
    assert {c["cls"] for c in cfgs} == {"PicardSolutionEnforceTerminal"}
    assert any(c["type"] == "Value" and c["scaler"][0] == "FixedLossScaler" for c in cfgs)


@pytest.mark.parametrize("name", CASES)
def test_terminal_fit_matches_reference_training_steps(name):
    f = _load(name)
    cfg = json.loads(str(f["cfg"]))
    nx, out_dim = cfg["nx"], cfg["output_dim"]
    assert out_dim == {"Value": 1, "OnlyGradient": nx}[cfg["type"]]
    dt = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        inner = construct_mlp(1 + nx, out_dim, cfg["neurons"], [cfg["act"]] * len(cfg["neurons"]), None)
        inner.load_state_dict({k[5:]: torch.from_numpy(v) for k, v in f.items() if k.startswith("init.")})
        e = cfg["eq"]
        net = PicardSolutionEnforceTerminal(eqs.Cha(e["nx"], e["alpha"], e["k"], e["T"]), inner, cfg["type"])
        assert net.T.dtype == torch.float64 and float(net.T) == e["T"]
        train = _train_cfg(cfg)
        objective, kind = F.build_objective(train, nx, True, False, out_dim)
        assert kind == {"Value": "gradient", "OnlyGradient": "head_only_gradient"}[cfg["type"]]
        opt, sched = F.make_optimizer(net.parameters(), train["OPTIMIZER"])
        batches = [(torch.from_numpy(f["tx"][s]), torch.from_numpy(f["y"][s])) for s in range(f["tx"].shape[0])]
        losses = F.train_steps(net, objective, opt, batches, sched).numpy()
        np.testing.assert_allclose(losses, f["losses"], rtol=1e-12, atol=0)
        for k, v in inner.state_dict().items():
            np.testing.assert_allclose(v.numpy(), f[f"final.{k}"], rtol=1e-9, atol=1e-12)
    finally:
        torch.set_default_dtype(dt)


def test_state_dict_is_the_references():
    """`model.*` and the buffer `T`: a reference checkpoint of the class loads unchanged."""
    net = PicardSolutionEnforceTerminal(eqs.Cha(4, 1.0, 5.0, 2.0), construct_mlp(5, 1, [8], ["Tanh"], None), "Value")
    assert set(net.state_dict()) == {"T", "model.0.weight", "model.0.bias", "model.2.weight", "model.2.bias"}
    assert float(net.T) == 2.0
    tx = torch.cat([torch.full((3, 1), 2.0), torch.randn(3, 4)], -1)  # u(T, x) = g(x) by construction
    assert torch.equal(net(tx), net.equation.g(tx[:, 1:]))
