"""The one case table of tests/test_net_weight_gates.py (CPU: every case passes net_weight.gate) and
tests/test_gpu_network_phase.py (MI355X: every case against the gate's reference at rel-L2 < 1e-4).

A case is a kernel instance x a net whose scales (hidden, out) were found on the CPU with the fp64
oracle (tools/search_net_weight.py) so that the gate holds; they stand in SCALES next to the net's id
and are not computed at test time.  Two cases that differ only in the GEMM mode share one net, one
gate and one reference.

Common shapes (tests/test_gpu_dispatch_rows.py): n = 3 points, M = 128 paths (two 64-path blocks per
point), K = 2 Euler steps, seed 1, epoch 1; torch.manual_seed(17) before every net, or the seed that
stands as a third entry next to its scales where no scales pass at seed 17: the net's last unit is all
but dead there, or (GBM at nx = 7, whose gradient label sees the network only through the change of f
along a path, while the equation's own value labels at these three points are small) the value share
leaves the band before the gradient share enters it."""
from collections import namedtuple

import numpy as np
import torch

import deeppicarditeration_amd as dpi
import net_weight as NW
from oracle import dpi_oracle as O

N, K, SEED, EPOCH, DT = 3, 2, 1, 1, 0.3
VG, OG = "ValueGradient", "OnlyGradient"

# group: unit / edge / hess / general / head / pis; variant: plain / td / wide / fb; head: None, VG, OG;
# mode: f32 / auto; v: SDGD samples (0: the full Hessian diagonal); fused: DPI_PIS_FUSED (None: default)
Case = namedtuple("Case", "group eq act widths nx variant head M v hess pis fused mode")


def _case(group, eq, act, widths, nx, mode, variant="plain", head=None, M=128, v=0, hess=False, pis=False, fused=None):
    return Case(group, eq, act, tuple(widths), nx, variant, head, M, v, hess, pis, fused, mode)


def _wid(w):
    return "x".join(map(str, w)) if len(set(w)) > 1 else f"{len(w)}x{w[0]}"


def net_id(c):
    """What the scales, the gate and the reference depend on: the case without its GEMM mode (and
    without DPI_PIS_FUSED, which selects launches, not numbers)."""
    parts = [c.group, c.eq, c.act, _wid(c.widths), f"nx{c.nx}"]
    parts += [c.variant] if c.variant != "plain" else []
    parts += [c.head] if c.head else []
    parts += [f"M{c.M}"] if c.M != 128 else []
    parts += [f"v{c.v}"] if c.v else []
    return "-".join(parts)


def case_id(c):
    return net_id(c) + ("-unfused" if c.fused == "0" else "") + "-" + c.mode


def _build():
    cases = []
    # every row of the unit table (csrc/dpi_route.h DPI_UNITS), as tests/test_gpu_dispatch_rows.py ROWS
    rows = [(eq, act, var) for var in ("plain", "td", "wide") for act in ("ELU", "Tanh") for eq in ("cha", "ou", "gbm")]
    rows += [("cha", "ELU", "fb"), ("ou", "ELU", "fb")]
    for eq, act, var in rows:
        nx = 129 if var == "wide" else 7
        cases.append(_case("unit", eq, act, [16], nx, "f32", var))  # only the fp32 instance exists
        cases += [_case("unit", eq, act, [32, 32], nx, mode, var) for mode in ("f32", "auto")]
    # the specialised width classes at their edges
    for mode in ("f32", "auto"):
        cases += [_case("edge", "cha", "ELU", [64, 64], nx, mode) for nx in (1, 7, 80, 96, 113, 128)]
        cases.append(_case("edge", "cha", "ELU", [128] * 4, 100, mode))
        cases.append(_case("edge", "ou", "ELU", [64] * 3, 100, mode))
        cases += [_case("edge", "gbm", "ELU", [64] * 3, 100, mode, v=v) for v in (100, 7)]
    cases.append(_case("edge", "cha", "ELU", [128] * 4, 100, "auto", M=100))
    cases.append(_case("edge", "ou", "ELU", [64] * 3, 100, "auto", M=100))
    cases.append(_case("edge", "gbm", "ELU", [64] * 3, 100, "auto", M=100, v=100))
    # Hessian labels
    for widths, nx in (([64] * 3, 100), ([32, 32], 7)):
        cases += [_case("hess", "gbm", act, widths, nx, mode, hess=True) for act in ("ELU", "Tanh")
                  for mode in ("f32", "auto")]
    # the general family (exact fp32 whatever the mode) and the gradient heads
    general = [[40], [129, 200, 256], [256] * 8, [100, 50, 20, 50, 100, 30, 10, 5], [17], [255, 1, 255]]
    for eq in ("cha", "ou"):
        for act in ("ELU", "Tanh"):
            cases += [_case("general", eq, act, w, 7, "auto") for w in general]
            cases += [_case("head", eq, act, w, 7, "auto", head=h) for h in (VG, OG) for w in general[:3]]
    cases.append(_case("general", "cha", "ELU", [256] * 8, 128, "auto"))
    cases.append(_case("general", "ou", "Tanh", [256] * 8, 128, "auto"))
    # PISGradNet (OU + GMM, nx = 100): k_pis_net<., NL> per depth; [32, 32] takes the layer-wise chain
    for mode in ("f32", "auto"):
        cases += [_case("pis", "ou", "ELU", [512] * L, 100, mode, pis=True) for L in (1, 2, 3, 4)]
        cases.append(_case("pis", "ou", "ELU", [32, 32], 100, mode, pis=True))
    cases.append(_case("pis", "ou", "ELU", [512] * 4, 100, "auto", pis=True, fused="0"))
    cases.append(_case("pis", "ou", "ELU", [512] * 4, 100, "auto", "td", pis=True))
    return cases


CASES = _build()

# net id -> (hidden_scale, out_scale[, net seed]), powers of two found by tools/search_net_weight.py: among
# the candidates that pass the gate, the one whose shares lie deepest inside [0.05, 0.95].  Beside each, as
# that search printed them (CPU-oracle figures): share value / grad[ / Hessian]; the weakest mutant and the
# largest rel-L2 by which it moves a block; the mutants exempt because their effect is exactly 0.0
SCALES = {
    "unit-cha-ELU-1x16-nx7": (1, 4),                        # 0.661 / 0.909; last_unit_last_layer 1.7e-03
    "unit-cha-ELU-2x32-nx7": (1, 2),                        # 0.133 / 0.375; unit_16 5.9e-02
    "unit-ou-ELU-1x16-nx7": (1, 16),                        # 0.456 / 0.572; last_unit_last_layer 1.5e-03; exempt out_bias
    "unit-ou-ELU-2x32-nx7": (1, 16),                        # 0.070 / 0.492; unit_16 1.1e-02; exempt out_bias
    "unit-gbm-ELU-1x16-nx7": (1, 4, 24),                    # 0.857 / 0.097; last_unit_last_layer 6.5e-02; exempt out_bias
    "unit-gbm-ELU-2x32-nx7": (4, 1, 18),                    # 0.763 / 0.056; unit_16 1.8e-02; exempt out_bias
    "unit-cha-Tanh-1x16-nx7": (1, 4),                       # 0.745 / 0.921; last_unit_last_layer 1.3e-03
    "unit-cha-Tanh-2x32-nx7": (2, 1),                       # 0.095 / 0.280; unit_16 3.9e-02
    "unit-ou-Tanh-1x16-nx7": (1, 16),                       # 0.375 / 0.377; last_unit_last_layer 1.4e-03; exempt out_bias
    "unit-ou-Tanh-2x32-nx7": (8, 4),                        # 0.110 / 0.345; unit_16 1.0e-01; exempt out_bias
    "unit-gbm-Tanh-1x16-nx7": (1, 4, 58),                   # 0.789 / 0.054; last_unit_last_layer 2.3e-02; exempt out_bias
    "unit-gbm-Tanh-2x32-nx7": (4, 1),                       # 0.872 / 0.055; last_unit_first_layer 2.4e-02; exempt out_bias
    "unit-cha-ELU-1x16-nx7-td": (1, 4),                     # 0.245 / 0.838; last_unit_last_layer 2.2e-03
    "unit-cha-ELU-2x32-nx7-td": (1, 1),                     # 0.218 / 0.395; unit_16 1.6e-02
    "unit-ou-ELU-1x16-nx7-td": (1, 32),                     # 0.753 / 0.718; last_unit_last_layer 1.5e-03
    "unit-ou-ELU-2x32-nx7-td": (1, 16),                     # 0.123 / 0.409; unit_16 8.6e-03
    "unit-gbm-ELU-1x16-nx7-td": (1, 2),                     # 0.863 / 0.367; last_unit_last_layer 1.9e-03
    "unit-gbm-ELU-2x32-nx7-td": (2, 0.5),                   # 0.192 / 0.187; last_x_column 9.6e-03
    "unit-cha-Tanh-1x16-nx7-td": (1, 4),                    # 0.342 / 0.788; last_unit_last_layer 1.4e-03
    "unit-cha-Tanh-2x32-nx7-td": (2, 0.5),                  # 0.140 / 0.337; unit_16 1.6e-02
    "unit-ou-Tanh-1x16-nx7-td": (1, 32),                    # 0.658 / 0.689; last_unit_last_layer 1.8e-03
    "unit-ou-Tanh-2x32-nx7-td": (1, 16),                    # 0.152 / 0.315; unit_16 5.2e-03
    "unit-gbm-Tanh-1x16-nx7-td": (1, 2),                    # 0.744 / 0.401; last_unit_last_layer 1.6e-03
    "unit-gbm-Tanh-2x32-nx7-td": (2, 0.5),                  # 0.258 / 0.179; unit_16 5.3e-03
    "unit-cha-ELU-1x16-nx129-wide": (1, 2),                 # 0.328 / 0.309; last_x_column 1.3e-02
    "unit-cha-ELU-2x32-nx129-wide": (1, 4),                 # 0.235 / 0.208; t_column 9.4e-03
    "unit-ou-ELU-1x16-nx129-wide": (1, 32),                 # 0.149 / 0.257; t_column 8.8e-03; exempt out_bias
    "unit-ou-ELU-2x32-nx129-wide": (2, 64),                 # 0.319 / 0.508; t_column 2.1e-02; exempt out_bias
    "unit-gbm-ELU-1x16-nx129-wide": (1, 4),                 # 0.253 / 0.103; last_unit_last_layer 1.4e-02; exempt out_bias
    "unit-gbm-ELU-2x32-nx129-wide": (2, 4),                 # 0.375 / 0.143; last_unit_last_layer 1.1e-02; exempt out_bias
    "unit-cha-Tanh-1x16-nx129-wide": (1, 2),                # 0.316 / 0.305; last_x_column 1.3e-02
    "unit-cha-Tanh-2x32-nx129-wide": (1, 4),                # 0.188 / 0.159; last_unit_last_layer 8.4e-03
    "unit-ou-Tanh-1x16-nx129-wide": (1, 64),                # 0.241 / 0.490; last_unit_last_layer 2.1e-02; exempt out_bias
    "unit-ou-Tanh-2x32-nx129-wide": (2, 64),                # 0.114 / 0.414; t_column 2.0e-02; exempt out_bias
    "unit-gbm-Tanh-1x16-nx129-wide": (1, 8),                # 0.502 / 0.149; last_x_column 1.2e-02; exempt out_bias
    "unit-gbm-Tanh-2x32-nx129-wide": (16, 0.125),           # 0.466 / 0.158; last_unit_last_layer 1.5e-02; exempt out_bias
    "unit-cha-ELU-1x16-nx7-fb": (1, 4),                     # 0.661 / 0.909; last_unit_last_layer 1.7e-03
    "unit-cha-ELU-2x32-nx7-fb": (1, 2),                     # 0.133 / 0.375; unit_16 5.9e-02
    "unit-ou-ELU-1x16-nx7-fb": (1, 16),                     # 0.456 / 0.572; last_unit_last_layer 1.5e-03; exempt out_bias
    "unit-ou-ELU-2x32-nx7-fb": (1, 16),                     # 0.070 / 0.492; unit_16 1.1e-02; exempt out_bias
    "edge-cha-ELU-2x64-nx1": (4, 0.125),                    # 0.321 / 0.145; out_bias 2.3e-03
    "edge-cha-ELU-2x64-nx7": (8, 0.125),                    # 0.244 / 0.187; out_bias 4.9e-03
    "edge-cha-ELU-2x64-nx80": (4, 2),                       # 0.121 / 0.474; out_bias 4.1e-02
    "edge-cha-ELU-2x64-nx96": (16, 0.5),                    # 0.104 / 0.408; out_bias 1.9e-02
    "edge-cha-ELU-2x64-nx113": (16, 0.5),                   # 0.077 / 0.354; out_bias 2.0e-02
    "edge-cha-ELU-2x64-nx128": (1, 4),                      # 0.117 / 0.249; t_column 6.5e-03
    "edge-cha-ELU-4x128-nx100": (2, 2),                     # 0.189 / 0.310; last_unit_last_layer 7.4e-03
    "edge-ou-ELU-3x64-nx100": (1, 128),                     # 0.173 / 0.295; t_column 1.9e-02; exempt out_bias
    "edge-gbm-ELU-3x64-nx100-v100": (8, 0.125),             # 0.237 / 0.218; last_unit_last_layer 6.0e-02; exempt out_bias
    "edge-gbm-ELU-3x64-nx100-v7": (16, 0.015625),           # 0.197 / 0.236; last_unit_last_layer 3.1e-02; exempt out_bias
    "edge-cha-ELU-4x128-nx100-M100": (2, 2),                # 0.187 / 0.304; last_unit_last_layer 7.3e-03
    "edge-ou-ELU-3x64-nx100-M100": (1, 128),                # 0.174 / 0.296; t_column 2.0e-02; exempt out_bias
    "edge-gbm-ELU-3x64-nx100-M100-v100": (8, 0.125),        # 0.233 / 0.249; last_unit_last_layer 7.5e-02; exempt out_bias
    "hess-gbm-ELU-3x64-nx100": (8, 0.0625),                 # 0.120 / 0.110 / 0.584; last_unit_first_layer 4.1e-01; exempt out_bias
    "hess-gbm-Tanh-3x64-nx100": (1, 64),                    # 0.392 / 0.135 / 0.375; unit_16 2.0e-02; exempt out_bias
    "hess-gbm-ELU-2x32-nx7": (4, 1, 18),                    # 0.763 / 0.055 / 0.224; last_unit_last_layer 4.1e-02; exempt out_bias
    "hess-gbm-Tanh-2x32-nx7": (4, 1),                       # 0.872 / 0.055 / 0.183; t_column 7.9e-02; exempt out_bias
    "general-cha-ELU-1x40-nx7": (1, 2),                     # 0.204 / 0.471; unit_16 2.1e-02
    "general-cha-ELU-129x200x256-nx7": (1, 4),              # 0.111 / 0.411; last_unit_last_layer 1.4e-02
    "general-cha-ELU-8x256-nx7": (4, 0.0625),               # 0.305 / 0.736; out_bias 2.3e-03
    "general-cha-ELU-100x50x20x50x100x30x10x5-nx7": (2, 0.5),# 0.204 / 0.234; out_bias 3.2e-02
    "general-cha-ELU-1x17-nx7": (1, 0.25),                  # 0.245 / 0.091; t_column 1.4e-02
    "general-cha-ELU-255x1x255-nx7": (1, 16),               # 0.274 / 0.461; out_bias 1.7e-03
    "head-cha-ELU-1x40-nx7-ValueGradient": (1, 1),          # 0.075 / 0.738; last_x_column 5.7e-02
    "head-cha-ELU-129x200x256-nx7-ValueGradient": (1, 2),   # 0.141 / 0.430; last_unit_first_layer 1.5e-02
    "head-cha-ELU-8x256-nx7-ValueGradient": (1, 8),         # 0.332 / 0.222; last_unit_last_layer 3.2e-03
    "head-cha-ELU-1x40-nx7-OnlyGradient": (1, 0.25),        # 0.127 / 0.254; unit_16 1.8e-02
    "head-cha-ELU-129x200x256-nx7-OnlyGradient": (8, 0.03125),# 0.115 / 0.381; last_unit_last_layer 1.6e-03
    "head-cha-ELU-8x256-nx7-OnlyGradient": (4, 0.0625),     # 0.912 / 0.931; last_unit_last_layer 1.2e-03
    "general-cha-Tanh-1x40-nx7": (1, 2),                    # 0.161 / 0.271; unit_16 2.2e-02
    "general-cha-Tanh-129x200x256-nx7": (1, 4),             # 0.135 / 0.332; last_unit_last_layer 1.4e-02
    "general-cha-Tanh-8x256-nx7": (1, 32),                  # 0.143 / 0.462; last_unit_first_layer 2.7e-02
    "general-cha-Tanh-100x50x20x50x100x30x10x5-nx7": (2, 0.5),# 0.153 / 0.229; last_unit_first_layer 2.6e-02
    "general-cha-Tanh-1x17-nx7": (1, 0.5),                  # 0.523 / 0.184; t_column 2.5e-02
    "general-cha-Tanh-255x1x255-nx7": (4, 8),               # 0.435 / 0.620; out_bias 1.7e-03
    "head-cha-Tanh-1x40-nx7-ValueGradient": (1, 2),         # 0.090 / 0.887; last_x_column 8.3e-02
    "head-cha-Tanh-129x200x256-nx7-ValueGradient": (1, 2),  # 0.140 / 0.441; last_unit_last_layer 2.3e-02
    "head-cha-Tanh-8x256-nx7-ValueGradient": (1, 8),        # 0.350 / 0.248; last_unit_last_layer 3.7e-03
    "head-cha-Tanh-1x40-nx7-OnlyGradient": (1, 0.25),       # 0.146 / 0.251; unit_16 1.7e-02
    "head-cha-Tanh-129x200x256-nx7-OnlyGradient": (2, 0.25),# 0.114 / 0.432; last_unit_last_layer 1.4e-03
    # the next net's last unit moves the label by < 1e-3 for hidden <= 4; at 16, eight saturated Tanh layers
    # amplify rounding: the fp64 oracle with its activations rounded to fp32 is already 6.2e-6 off on the gradient
    # block (9e-8 for the ELU twin), and the exact-fp32 kernel measures 4.9e-5 there, the suite's largest
    "head-cha-Tanh-8x256-nx7-OnlyGradient": (16, 0.5),      # 0.071 / 0.641; last_unit_last_layer 1.3e-03
    "general-ou-ELU-1x40-nx7": (1, 16),                     # 0.153 / 0.587; unit_16 1.3e-02; exempt out_bias
    "general-ou-ELU-129x200x256-nx7": (16, 0.125),          # 0.229 / 0.410; last_unit_last_layer 1.5e-02; exempt out_bias
    "general-ou-ELU-8x256-nx7": (2, 8),                     # 0.174 / 0.309; unit_16 2.1e-02; exempt out_bias
    "general-ou-ELU-100x50x20x50x100x30x10x5-nx7": (1, 1024),# 0.202 / 0.315; last_unit_first_layer 1.7e-02; exempt out_bias
    "general-ou-ELU-1x17-nx7": (1, 8),                      # 0.204 / 0.569; t_column 3.1e-02; exempt out_bias
    "general-ou-ELU-255x1x255-nx7": (1, 64),                # 0.160 / 0.222; last_unit_last_layer 1.0e-02; exempt out_bias
    "head-ou-ELU-1x40-nx7-ValueGradient": (1, 2),           # 0.061 / 0.433; unit_16 2.5e-02
    "head-ou-ELU-129x200x256-nx7-ValueGradient": (1, 4),    # 0.108 / 0.454; last_unit_first_layer 1.5e-02
    "head-ou-ELU-8x256-nx7-ValueGradient": (1, 16),         # 0.220 / 0.460; unit_16 5.3e-03
    "head-ou-ELU-1x40-nx7-OnlyGradient": (1, 1),            # 0.161 / 0.481; t_column 3.5e-02
    "head-ou-ELU-129x200x256-nx7-OnlyGradient": (2, 1),     # 0.095 / 0.412; last_unit_last_layer 1.4e-02
    "head-ou-ELU-8x256-nx7-OnlyGradient": (1, 16),          # 0.119 / 0.366; unit_16 1.6e-03
    "general-ou-Tanh-1x40-nx7": (1, 16),                    # 0.112 / 0.430; unit_16 1.7e-02; exempt out_bias
    "general-ou-Tanh-129x200x256-nx7": (1, 32),             # 0.180 / 0.394; last_unit_last_layer 1.6e-02; exempt out_bias
    "general-ou-Tanh-8x256-nx7": (1, 512),                  # 0.378 / 0.350; unit_16 1.2e-02; exempt out_bias
    "general-ou-Tanh-100x50x20x50x100x30x10x5-nx7": (1, 512),# 0.145 / 0.200; last_unit_first_layer 2.2e-02; exempt out_bias
    "general-ou-Tanh-1x17-nx7": (1, 8),                     # 0.156 / 0.352; t_column 5.5e-02; exempt out_bias
    "general-ou-Tanh-255x1x255-nx7": (1, 256),              # 0.195 / 0.500; last_unit_first_layer 1.9e-02; exempt out_bias
    "head-ou-Tanh-1x40-nx7-ValueGradient": (1, 4),          # 0.301 / 0.743; unit_16 6.2e-02
    "head-ou-Tanh-129x200x256-nx7-ValueGradient": (1, 4),   # 0.112 / 0.362; last_unit_last_layer 1.5e-02
    "head-ou-Tanh-8x256-nx7-ValueGradient": (1, 16),        # 0.223 / 0.467; last_unit_first_layer 4.9e-03
    "head-ou-Tanh-1x40-nx7-OnlyGradient": (1, 1),           # 0.133 / 0.353; t_column 1.4e-02
    "head-ou-Tanh-129x200x256-nx7-OnlyGradient": (4, 1),    # 0.114 / 0.423; last_unit_last_layer 2.4e-02
    "head-ou-Tanh-8x256-nx7-OnlyGradient": (1, 16),         # 0.113 / 0.353; unit_16 2.4e-03
    "general-cha-ELU-8x256-nx128": (2, 1),                  # 0.201 / 0.316; last_unit_last_layer 1.2e-03
    "general-ou-Tanh-8x256-nx128": (2, 64),                 # 0.143 / 0.388; last_unit_last_layer 2.0e-03; exempt out_bias
    "pis-ou-ELU-1x512-nx100": (1, 16, 23),                  # 0.263 / 0.888; t_encoder_last_unit 3.8e-03; exempt smooth_last_row
    "pis-ou-ELU-2x512-nx100": (2, 16),                      # 0.074 / 0.710; t_encoder_last_unit 1.9e-03; exempt smooth_last_row
    "pis-ou-ELU-3x512-nx100": (16, 0.5),                    # 0.067 / 0.809; t_encoder_last_unit 7.3e-03; exempt smooth_last_row
    "pis-ou-ELU-4x512-nx100": (8, 1),                       # 0.070 / 0.725; last_unit_first_layer 9.7e-03; exempt smooth_last_row
    "pis-ou-ELU-2x32-nx100": (1, 32),                       # 0.059 / 0.621; t_column 2.0e-03; exempt smooth_last_row
    "pis-ou-ELU-4x512-nx100-td": (4, 8),                    # 0.079 / 0.578; t_encoder_last_unit 2.1e-03; exempt smooth_last_row
}


def scales(c):
    return SCALES[net_id(c)]


# ----------------------------------------------------------------------------- builders
def equations(c):
    """(product equation, oracle equation).  Small problems as tests/test_gpu_dispatch_rows.py draws
    them; the PISGradNet cases on the shipped 5-component mixture of BASELINE configs[2]."""
    nx = c.nx
    if c.pis:
        eq = dpi.OUProcessEquation(nx=nx, T=1.0, alpha=1.0, num_components=5, mean_scale=1.0, var_scale=2.0,
                                   alpha_scale=4.0)
        return eq, O.OUProcessEquation(nx, eq.mean.numpy(), eq.var.numpy(), eq.pi.numpy(), alpha_scale=4.0)
    rng = np.random.default_rng(nx)
    if c.eq == "cha":
        return dpi.Cha(nx, 1.0, 5.0, 1.0), O.Cha(nx, 1.0, 5.0, 1.0)
    if c.eq == "ou":
        C = 3
        mean, var, pi = rng.uniform(-1, 1, (C, nx)), np.full((C, nx), 2.0), rng.uniform(0.1, 1, C)
        pi = pi / pi.sum()
        eq = dpi.OUProcessEquation(nx=nx, T=1.0, alpha=1.0, num_components=C, mean=mean, var=var, pi=pi, alpha_scale=4.0)
        return eq, O.OUProcessEquation(nx, mean, var, pi, alpha_scale=4.0)
    w = rng.standard_normal((2, 1 + nx)) / np.sqrt(nx)
    w[:, 0] = 1.0
    eq = dpi.GBMEquationComplexExact(nx, 1.0, 1.0, w=w, v=rng.standard_normal((2, 1)))
    return eq, O.GBMEquationComplexExact(nx, eq.w.numpy(), eq.v.numpy())


NET_SEED = 17


def default_module(c, eq, seed=NET_SEED):
    """The case's net at torch's default initialisation."""
    torch.manual_seed(seed)
    if c.pis:
        m = dpi.PISGradNet(hidden_shapes=list(c.widths), dim=c.nx, g0=eq.g, T=1.0)
        with torch.no_grad():
            m.timestep_phase.copy_(0.1 * torch.randn(1, 64))
        return m
    n_out = {None: 1, VG: 1 + c.nx, OG: c.nx}[c.head]
    return dpi.construct_mlp(1 + c.nx, n_out, list(c.widths), [c.act] * len(c.widths), None)


def network(c, eq, oeq, scales_=None):
    """(module, oracle twin) of the case at its scales (hidden, out[, torch seed of the net])."""
    h, o, *seed = scales(c) if scales_ is None else scales_
    return NW.weighted_mlp(default_module(c, eq, *seed), h, o, oeq=oeq)


def oracle_kw(c):
    """The oracle arguments after (oeq, onet, tx) of NW.gate / NW.labels."""
    return dict(M=c.M, K=K, seed=SEED, epoch=EPOCH, v=c.v, delta_t=DT if c.variant == "td" else 0.0, hessians=c.hess)


_REFERENCES = {}


def reference(c, oeq, onet, tx, info=None, with_mutants=True):
    """NW.gate's reference labels for the case at points tx, computed (and gated) once per net and
    points: the f32 and auto case of one net label the same points."""
    tx = np.asarray(tx, np.float64)
    key = (net_id(c), tx.tobytes(), with_mutants)
    if key not in _REFERENCES:
        inf = {}
        ref = NW.gate(oeq, onet, tx, info=inf, with_mutants=with_mutants, **oracle_kw(c))
        ref.setflags(write=False)
        _REFERENCES[key] = (ref, inf)
    ref, inf = _REFERENCES[key]
    if info is not None:
        info.update(inf)
    return ref
