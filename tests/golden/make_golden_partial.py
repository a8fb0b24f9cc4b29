"""Golden label vectors at Monte-Carlo sample counts that are no multiple of the 64-path block,
from the REFERENCE implementation, into tests/golden/partial/.

The same procedure as make_golden.py (whose run_case this calls; it needs the reference checkout
that module names): the reference's OnlineDataGenerator run with the oracle's Philox noise injected
in its draw order.  The fixtures live in a sub-folder because golden_util's glob is not recursive:
the tests parametrised over tests/golden/*.npz build the strict generator (multiples of 64 only)
and must not pick these up; golden_util.load("partial/<name>") reads them.

Usage:  python tests/golden/make_golden_partial.py
"""
import shutil

import make_golden as G

CHA = {"nx": 100, "alpha": 1.0, "k": 5.0, "T": 1.0}
OU = {"nx": 100, "alpha": 1.0, "T": 1.0, "num_components": 5, "mean_scale": 1.0, "var_scale": 2.0,
      "alpha_scale": 4.0}
GBM = {"nx": 100, "alpha": 1.0, "T": 1.0}


def main():
    (G.HERE / "partial").mkdir(exist_ok=True)
    wd = G.prepare_workdir()
    # one full block and a 36-lane tail; a single path (63 dead lanes)
    G.run_case("partial/cha_mlp16_M100_K2", "Cha", CHA, "mlp", {"neurons": [16, 16]}, 3, 100, 2, 91, workdir=wd)
    G.run_case("partial/cha_mlp16_M1_K2", "Cha", CHA, "mlp", {"neurons": [16, 16]}, 3, 1, 2, 92, epoch=1, workdir=wd)
    # PISGradNet: a tail of one live row
    G.run_case("partial/ou_pis32_M65_K2", "OUProcessEquation", OU, "pis", {"neurons": [32, 32]}, 2, 65, 2, 93,
               workdir=wd)
    # unequal counts, both ragged (terminal 37, integral 100), full Hessian diagonal
    G.run_case("partial/gbm_mlp32x3_M100_MT37_K2", "GBMEquationComplexExact", GBM, "mlp", {"neurons": [32] * 3}, 2,
               100, 2, 94, workdir=wd, MT=37)
    # Malliavin Hessian labels
    G.run_case("partial/gbm_hess_mlp32x3_M100_K2", "GBMEquationComplexExact", GBM, "mlp", {"neurons": [32] * 3}, 2,
               100, 2, 95, workdir=wd, hessians=True)
    shutil.rmtree(wd)


if __name__ == "__main__":
    main()
