"""TRAIN.CORE_FORM and the form of the PISGradNet core it selects (config.py, fit.build_objective,
fit.device_objective) — CPU only.  "tiles", the default, builds what was built before the key existed; "layers",
under TRAIN.BACKEND: hip, hands the layer-wise C entries to `_PISCore`, and what the form does not cover is
refused by name: at configuration load where the configuration shows it, otherwise at the first batch before
the library is touched."""
import pytest
import torch

import pis_fit_reference as R
from deeppicarditeration_amd import _lib, fit
from deeppicarditeration_amd.config import get_default_cfg, load_cfg
from deeppicarditeration_amd.solution import PISGradNet, construct_mlp


def _yaml(tmp_path, train=""):
    f = tmp_path / "a.yaml"
    f.write_text(f"NAME: x\nTRAIN: {{{train}}}\n")
    return str(f)


def _eq(nx=4):
    return R.make_equation((3, nx, [16], 1.0, 0.0, False, 1.0))


def test_key_defaults_to_tiles_and_loads(tmp_path):
    assert get_default_cfg().TRAIN.CORE_FORM == "tiles"
    assert load_cfg(_yaml(tmp_path)).TRAIN.CORE_FORM == "tiles"
    assert load_cfg(_yaml(tmp_path, "BACKEND: hip")).TRAIN.CORE_FORM == "tiles"
    assert load_cfg(_yaml(tmp_path, "BACKEND: hip, CORE_FORM: layers")).TRAIN.CORE_FORM == "layers"
    assert load_cfg(_yaml(tmp_path, "BACKEND: hip"), ["TRAIN.CORE_FORM", "layers"]).TRAIN.CORE_FORM == "layers"
    assert load_cfg(_yaml(tmp_path, "BACKEND: hip, CORE_FORM: layers"),
                    ["TRAIN.CORE_FORM", "tiles"]).TRAIN.CORE_FORM == "tiles"
    assert load_cfg(_yaml(tmp_path, "CORE_FORM: tiles")).TRAIN.CORE_FORM == "tiles"  # the default under torch too
    for bad in ("rows", "Layers", "1"):
        with pytest.raises(ValueError, match="TRAIN.CORE_FORM"):
            load_cfg(_yaml(tmp_path, f"BACKEND: hip, CORE_FORM: {bad}"))


def test_layers_under_the_torch_backend_is_refused_at_load(tmp_path):
    for train in ("CORE_FORM: layers", "BACKEND: torch, CORE_FORM: layers"):
        with pytest.raises(NotImplementedError, match="TRAIN.CORE_FORM") as e:
            load_cfg(_yaml(tmp_path, train))
        assert "TRAIN.BACKEND: torch" in str(e.value)
    with pytest.raises(NotImplementedError, match="TRAIN.CORE_FORM") as e:
        fit.build_objective(get_default_cfg().TRAIN, 4, True, False, backend="torch", core_form="layers")
    assert "TRAIN.BACKEND: torch" in str(e.value)
    with pytest.raises(ValueError, match="TRAIN.CORE_FORM"):
        fit.build_objective(get_default_cfg().TRAIN, 4, True, False, backend="hip", core_form="rows")


def test_build_objective_hands_the_form_to_the_device_objective(monkeypatch):
    """The same closure and the same kinds as today; the form arrives at `_PISPlan`, which names the layer-wise
    entries for `_PISCore`.  The CPU batch is then the error: nothing falls back to torch."""
    t = get_default_cfg().TRAIN
    for sg, want in ((False, "value"), (True, "gradient")):
        obj, kind = fit.build_objective(t, 4, sg, False, backend="hip", core_form="layers")
        assert kind == want and obj.__qualname__.startswith("device_objective.")
    seen = []
    plan_cls = fit._PISPlan

    class Plan(plan_cls):
        def __init__(self, *args):
            seen.append(args[2:])
            super().__init__(*args)

    monkeypatch.setattr(fit, "_PISPlan", Plan)
    net = PISGradNet([16], 4, _eq().g)
    with pytest.raises(_lib.DPIError, match="no CPU fallback"):
        obj(net, torch.zeros(3, 5), torch.zeros(3, 5))
    assert seen == [("layers",)]
    plan = plan_cls(net, 4, "layers")
    assert (plan.ws_bytes, plan.forward, plan.backward) == ("dpi_fit_core_layers_workspace_bytes",
                                                            "dpi_fit_core_layers_forward",
                                                            "dpi_fit_core_layers_backward")
    assert {plan.ws_bytes, plan.forward, plan.backward} <= set(_lib.SIGNATURES)
    # what _PISPlan refuses stays refused, with its text
    with pytest.raises(NotImplementedError, match="PISGradNet NETWORK.NEURONS"):
        plan_cls(PISGradNet([8] * 5, 4, _eq().g), 4, "layers")
    with pytest.raises(ValueError, match="TRAIN.CORE_FORM"):
        plan_cls(net, 4, "rows")


def test_a_construct_mlp_net_under_layers_is_refused_by_name_at_the_first_batch(monkeypatch):
    """No GPU and no library: the network is looked at before either is touched."""
    monkeypatch.setattr(_lib, "load", lambda *a, **k: pytest.fail("the library was touched"))
    net = construct_mlp(5, 1, [8, 8], ["ELU", "ELU"], None)
    obj = fit.device_objective(0.0, torch.square, fit.FixedLossScaler(1.0), 4, core_form="layers")
    with pytest.raises(NotImplementedError, match="TRAIN.CORE_FORM") as e:
        obj(net, torch.zeros(3, 5), torch.zeros(3, 5))
    assert "layers" in str(e.value) and "PISGradNet" in str(e.value)
    step = fit.device_step(0.0, torch.square, fit.FixedLossScaler(1.0), 4, core_form="layers")
    with pytest.raises(NotImplementedError, match="TRAIN.CORE_FORM"):
        step(net, torch.optim.Adam(net.parameters()), torch.zeros(3, 5), torch.zeros(3, 5))


def test_the_default_form_builds_what_it_built_before(monkeypatch):
    """No core_form, or "tiles": device_objective is called with today's four arguments, `_PISPlan` names
    dpi_fit_core_*, and a construct_mlp net takes `_DevicePlan` as before."""
    calls = []
    real = fit.device_objective

    def recording(*args, **kwargs):
        calls.append((len(args), kwargs))
        return real(*args, **kwargs)

    monkeypatch.setattr(fit, "device_objective", recording)
    t = get_default_cfg().TRAIN
    for form in ({}, {"core_form": "tiles"}):
        obj, kind = fit.build_objective(t, 4, True, False, backend="hip", **form)
        assert kind == "gradient" and obj.__qualname__.startswith("device_objective.")
    assert calls == [(4, {}), (4, {})]
    net = PISGradNet([16], 4, _eq().g)
    plan = fit._PISPlan(net, 4)
    assert plan.core_form == "tiles"
    assert (plan.ws_bytes, plan.forward, plan.backward) == ("dpi_fit_core_workspace_bytes", "dpi_fit_core_forward",
                                                            "dpi_fit_core_backward")
    with pytest.raises(_lib.DPIError, match="no CPU fallback"):
        obj(net, torch.zeros(3, 5), torch.zeros(3, 5))
    mlp = construct_mlp(5, 1, [8, 8], ["ELU", "ELU"], None)
    with pytest.raises(_lib.DPIError):  # _DevicePlan accepted it; the CPU batch (or a missing library) is the error
        obj(mlp, torch.zeros(3, 5), torch.zeros(3, 5))
