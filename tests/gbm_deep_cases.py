"""The case table of the general MLP family on GBM (csrc/dpi_general_gbm.h): GBMEquationComplexExact with
value nets of 1..8 hidden layers, widths <= 64, that have no specialised GBM instance.  Used by
tests/test_gbm_deep_gates.py (CPU: every case passes net_weight.gate) and tests/test_gpu_gbm_deep.py
(MI355X: every case against the gate's reference at rel-L2 < 1e-4, and the structure tests).

Built on tests/net_weight_cases.py: the same Case, ids, equations, nets and oracle arguments; only the
cases and their scales are this module's.  tools/search_net_weight.py --cases gbm_deep_cases finds the
scales.  Shapes as there: n = 3 points, M = 128 (two blocks per point), K = 2, seed 1, epoch 1; nx = 7
unless the case says otherwise; v: SDGD samples (0: the exact diagonal)."""
import net_weight_cases as T
from net_weight_cases import (EPOCH, K, N, SEED, Case, case_id, default_module, equations, net_id,  # noqa: F401
                              oracle_kw, reference)

IRREGULAR = [33, 64, 20, 48, 10]  # the widest layer is not the first; 33 and 20 are no multiple of 16


def _c(act, widths, nx=7, v=0, M=128):
    return T._case("gbmgen", "gbm", act, widths, nx, "auto", M=M, v=v)


CASES = [
    _c("Tanh", [64] * 4),
    _c("ELU", [64] * 4),
    _c("Tanh", [64] * 8, v=7),  # v = nx = 7 with replacement
    _c("ELU", [64] * 8, v=7),
    _c("ELU", [16] * 5, v=7),
    _c("Tanh", [16] * 5, v=7),
    _c("ELU", [32] * 4, v=7),
    _c("ELU", IRREGULAR),
    _c("Tanh", IRREGULAR),
    _c("Tanh", [40], v=7),  # L = 1, the (64, 1) class
    _c("ELU", [64] * 4, nx=100, v=100),
    _c("ELU", [64] * 5, nx=100, M=100, v=100),  # a partial block
    _c("ELU", [64] * 4, nx=128, v=7),
    _c("Tanh", [64] * 8, nx=100, v=7),
]

# net id -> (hidden scale, out scale, torch seed of the net): powers of two found by the search, with the
# share value / grad it printed (CPU-oracle figures)
SCALES = {
    "gbmgen-gbm-Tanh-4x64-nx7": (8, 1 / 64, 17),                   # 0.645 / 0.092
    "gbmgen-gbm-ELU-4x64-nx7": (4, 1 / 8, 19),                     # 0.734 / 0.056
    "gbmgen-gbm-Tanh-8x64-nx7-v7": (4, 1 / 64, 18),                # 0.698 / 0.202
    "gbmgen-gbm-ELU-8x64-nx7-v7": (2, 2, 58),                      # 0.911 / 0.090
    "gbmgen-gbm-ELU-5x16-nx7-v7": (2, 1, 17),                      # 0.659 / 0.054
    "gbmgen-gbm-Tanh-5x16-nx7-v7": (4, 1 / 16, 18),                # 0.473 / 0.064
    "gbmgen-gbm-ELU-4x32-nx7-v7": (4, 1 / 8, 23),                  # 0.710 / 0.059
    "gbmgen-gbm-ELU-4x64-nx128-v7": (2, 2, 17),                    # 0.179 / 0.178
    "gbmgen-gbm-ELU-33x64x20x48x10-nx7": (2, 2, 17),              # 0.840 / 0.058
    "gbmgen-gbm-Tanh-33x64x20x48x10-nx7": (2, 2, 17),              # 0.923 / 0.079
    "gbmgen-gbm-Tanh-1x40-nx7-v7": (1, 4, 18),                     # 0.818 / 0.054
    "gbmgen-gbm-ELU-4x64-nx100-v100": (8, 1 / 32, 17),             # 0.367 / 0.296
    "gbmgen-gbm-ELU-5x64-nx100-M100-v100": (4, 1 / 8, 17),         # 0.272 / 0.222
    "gbmgen-gbm-Tanh-8x64-nx100-v7": (4, 1 / 32, 17),              # 0.184 / 0.214
}


def scales(c):
    return SCALES[net_id(c)]


def network(c, eq, oeq, scales_=None):
    return T.network(c, eq, oeq, scales(c) if scales_ is None else scales_)
