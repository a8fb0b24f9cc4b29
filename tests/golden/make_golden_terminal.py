"""Golden label vectors of terminal-enforcing solutions (NETWORK.cls PicardSolutionEnforceTerminal) from
the REFERENCE implementation, written to tests/golden/terminal/*.npz (a folder of its own: every .npz
directly under tests/golden/ is a case of the value-network parity tests).

Runs only where the reference is present; the module stand-ins, the noise injection and the draw
order are make_golden.py's.  Each case builds the reference's own
PicardSolutionEnforceTerminal(eq, network_cfg, train_cfg) (picard/solution_enforce_terminal.py:9-27:
u = g + (T - t) N for NETWORK.TYPE Value, g_x + (T - t) N with nx outputs for OnlyGradient) and feeds
it to the reference's OnlineDataGenerator.sample_with_gradients.  Outputs are data only: inputs, the
inner network's weights, expected labels.

Usage:  python tests/golden/make_golden_terminal.py
"""
import importlib
import shutil
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
import make_golden as mg  # noqa: E402  (installs the stand-ins, imports the reference)

set_mod = importlib.import_module("picard.solution_enforce_terminal")
OUT = HERE / "terminal"


def run_case(name, eq_name, eq_kw, typ, neurons, act, n, M, K, seed, epoch=0, point_base=0, init_seed=0, workdir=None):
    torch.set_default_dtype(torch.float64)
    eq = mg.make_equation(eq_name, eq_kw, workdir)
    torch.manual_seed(init_seed)
    ncfg = mg.CfgNode({"TYPE": typ, "PISGRADNET": False, "NEURONS": neurons, "ACTIVATIONS": [act] * len(neurons),
                       "BOUND": None})
    tcfg = mg.CfgNode({"LOSS": mg.CfgNode({"beta": 0.0, "FN": mg.CfgNode({"cls": None})})})
    sol = set_mod.PicardSolutionEnforceTerminal(eq, ncfg, tcfg)
    hess = mg.CfgNode({"method": None, "kwargs": mg.CfgNode({})})
    gen = mg.data.OnlineDataGenerator(eq, sol, 1, 1, device="cpu", t_always_uniform=True, n_estimate_terminal=M,
                                      n_estimate_integral=M, hessian_approximation=hess, sample_bound=None,
                                      estimate_terminal="OU_ByGx", estimate_integral="OU_Simple", estimate_delta_t=0.0)
    with mg.NoiseQueue(mg.noise_items(eq_name, eq.nx, n, M, K, seed, epoch, point_base, 0)):
        tx, y = gen.sample_with_gradients(n)
    out = {"case": name, "eq": eq_name, "net": "mlp", "type": typ, "cls": type(sol).__name__, "n": n, "M": M, "K": K,
           "seed": np.uint64(seed), "epoch": epoch, "point_base": point_base, "tx": tx.numpy(), "y": y.detach().numpy(),
           "neurons": np.asarray(neurons), "acts": np.asarray([act] * len(neurons))}
    for k, val in eq_kw.items():
        out[f"eqkw_{k}"] = val
    for k, val in mg.state_dict_np(sol.model).items():
        out[f"sd_{k}"] = val
    if eq_name == "OUProcessEquation":
        out["gmm_mean"] = eq.mean.numpy()
        out["gmm_var"] = torch.diagonal(eq.var, dim1=1, dim2=2).numpy()
        out["gmm_pi"] = eq.pi.numpy()
    OUT.mkdir(exist_ok=True)
    np.savez_compressed(OUT / f"{name}.npz", **out)
    print(f"{name}: tx {tx.shape} y {y.shape} |y|={float(y.norm()):.4g}")


def main():
    wd = mg.prepare_workdir()
    cha = {"nx": 100, "alpha": 1.0, "k": 5.0, "T": 1.0}
    ou = {"nx": 100, "alpha": 1.0, "T": 1.0, "num_components": 5, "mean_scale": 1.0, "var_scale": 2.0,
          "alpha_scale": 4.0}
    seed = 200
    for eq_tag, eq_name, kw in (("cha", "Cha", cha), ("ou", "OUProcessEquation", ou)):
        for typ, ttag in (("Value", "v"), ("OnlyGradient", "og")):
            for act, neurons, K in (("ELU", [16, 16], 2), ("Tanh", [24] * 3, 1)):
                seed += 1
                tag = "x".join(map(str, neurons))
                run_case(f"{eq_tag}_{ttag}_{act.lower()}_{tag}_K{K}", eq_name, kw, typ, neurons, act, 3, 64, K, seed,
                         epoch=seed % 3, point_base=seed % 5, workdir=wd)
    cha7 = {**cha, "nx": 7}
    run_case("cha7_v_tanh_20x20_K2", "Cha", cha7, "Value", [20, 20], "Tanh", 3, 64, 2, 231, workdir=wd)
    run_case("cha7_og_elu_20x20_K2", "Cha", cha7, "OnlyGradient", [20, 20], "ELU", 3, 64, 2, 232, epoch=1, workdir=wd)
    shutil.rmtree(wd)


if __name__ == "__main__":
    main()
