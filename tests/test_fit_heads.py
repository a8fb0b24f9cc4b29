"""The outer fit of gradient-head networks (NETWORK.TYPE ValueGradient / OnlyGradient) against the
reference's own training steps (tests/golden/fit_heads/*.npz, made by
tests/golden/make_fit_golden_heads.py from picard/solution_jac.py:167-213): same initial weights, same
batches, same optimizer -> the per-step losses agree to rtol 1e-12 and the final weights to fp64
rounding, the bars of tests/test_fit_golden.py.  CPU, fp64."""
import json
from pathlib import Path

import numpy as np
import pytest
import torch

from deeppicarditeration_amd import fit as F
from deeppicarditeration_amd.solution import construct_mlp

DIR = Path(__file__).parent / "golden" / "fit_heads"
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
                     "use_aux_loss": cfg["use_aux_loss"], "weight_aux_loss": cfg["weight_aux_loss"]},
            "NUM_HESS_SAMPLES": -1, "OPTIMIZER": {"cls": "Adam", "kwargs": {"lr": cfg["lr"]}}}


def test_fixture_set():
    cfgs = [json.loads(str(_load(c)["cfg"])) for c in CASES]
    assert {c["type"] for c in cfgs} == {"ValueGradient", "OnlyGradient"}
    assert any(c["use_aux_loss"] for c in cfgs)
    assert any(c["scaler"] and c["scaler"][0] != "FixedLossScaler" for c in cfgs)


@pytest.mark.parametrize("name", CASES)
def test_head_fit_matches_reference_training_steps(name):
    f = _load(name)
    cfg = json.loads(str(f["cfg"]))
    nx, out_dim = cfg["nx"], cfg["output_dim"]
    assert out_dim == {"ValueGradient": 1 + nx, "OnlyGradient": nx}[cfg["type"]]
    dt = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        net = construct_mlp(1 + nx, out_dim, cfg["neurons"], [cfg["act"]] * len(cfg["neurons"]), None)
        net.load_state_dict({k[5:]: torch.from_numpy(v) for k, v in f.items() if k.startswith("init.")})
        train = _train_cfg(cfg)
        objective, kind = F.build_objective(train, nx, True, False, out_dim)
        assert kind == {"ValueGradient": "head_value_gradient", "OnlyGradient": "head_only_gradient"}[cfg["type"]]
        opt, sched = F.make_optimizer(net.parameters(), train["OPTIMIZER"])
        batches = [(torch.from_numpy(f["tx"][s]), torch.from_numpy(f["y"][s])) for s in range(f["tx"].shape[0])]
        losses = F.train_steps(net, objective, opt, batches, sched).numpy()
        np.testing.assert_allclose(losses, f["losses"], rtol=1e-12, atol=0)
        for k, v in net.state_dict().items():
            np.testing.assert_allclose(v.numpy(), f[f"final.{k}"], rtol=1e-9, atol=1e-12)
    finally:
        torch.set_default_dtype(dt)


def test_only_gradient_has_no_value_loss():
    nx = 5
    torch.manual_seed(0)
    net = construct_mlp(1 + nx, nx, [8], ["Tanh"], None)
    obj, _ = F.build_objective({"LOSS": {"beta": 0.0}}, nx, True, False, nx)
    _, info = obj(net, torch.randn(4, 1 + nx), torch.randn(4, 1 + nx))
    assert float(info["train_value_loss"]) == 0.0


def test_refusals_by_name():
    fixed = {"LOSS": {"beta": 0.0, "SCALER": {"cls": "FixedLossScaler", "kwargs": {"fixed_weight": 1e-9}}}}
    with pytest.raises(NotImplementedError, match="fixed_weight"):
        F.build_objective(fixed, 4, True, False, 5)
    with pytest.raises(NotImplementedError, match="SUPERVISE_HESSIAN"):
        F.build_objective({"LOSS": {"beta": 0.0}}, 4, True, True, 4)
    aux = {"LOSS": {"beta": 0.0, "use_aux_loss": True, "weight_aux_loss": 0.1}}
    with pytest.raises(NotImplementedError, match="use_aux_loss"):
        F.build_objective(aux, 4, True, False, 4)  # OnlyGradient
    with pytest.raises(NotImplementedError, match="use_aux_loss"):
        F.build_objective(aux, 4, True, False)  # Value
    assert F.build_objective(aux, 4, True, False, 5)[1] == "head_value_gradient"
    with pytest.raises(ValueError, match="output width"):
        F.build_objective({"LOSS": {"beta": 0.0}}, 4, True, False, 3)
