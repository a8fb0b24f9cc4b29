"""The cases of tests/test_gpu_noise_table.py (the per-wave Philox table of the first-order rollouts:
csrc/dpi_rng.h NOISE_TABLE, the overlay on the weight ring in csrc/dpi_device.h paths_body), shared
with tools/record_noise_table_golden.py, which records the labels the bitwise test pins.

Cha, 2 points, M = 128 (two 64-path blocks per point) unless a case says otherwise.  Shapes: the
smallest at which the chunked loop and the overlay can go wrong —
  K = 1 one entry, 3 the remainder loop only, 4 one unrolled group, 64 one full chunk, 65 a second
  chunk of one entry, 130 three chunks and a remainder (at nx = 100 only);
  nx = 4 one dim-block (three waves skip the rollout and reach the barriers first), 100 the 13/12/12/13
  skew of the flagship workload, 128 every wave full (at K = 65).
Nets: 4 x 128 ELU on the fp16-split MFMA (the ring is used by LDS-DMA right after and right before a
rollout) and in exact fp32 (the same, with staged fp32 chunks), and ZeroSolution (no ring use).
One OU case (MLP 2 x 64, nx = 100, K = 65) and one with M = 100 (dead lanes in the last block).

The MLP weights come from the oracle's integer Philox, scaled by a power of two: the same bits on
every host, so the recorded labels stay comparable."""
import numpy as np
import torch

import deeppicarditeration_amd as dpi
from deeppicarditeration_amd import _lib as L
from oracle import dpi_oracle as O
from oracle import philox as PH

N_POINTS, SEED, EPOCH = 2, 11, 2
ENTRIES = ("sample", "generate")  # sample_with_gradients (k_paths_fb), generate_with_gradients (k_paths)

SHAPES = [(K, nx) for K in (1, 3, 4, 64, 65) for nx in (4, 100)] + [(130, 100), (65, 128)]
NETS = ("mlp128x4-split", "mlp128x4-f32", "zero")
# id -> (equation, nx, K, M, net)
CASES = {f"cha{nx}_K{K}_{net}": ("cha", nx, K, 128, net) for K, nx in SHAPES for net in NETS}
CASES["ou100_K65_mlp64x2-split"] = ("ou", 100, 65, 128, "mlp64x2-split")
CASES["cha100_K65_M100_mlp128x4-split"] = ("cha", 100, 65, 100, "mlp128x4-split")
# the bitwise test's subset: every ZeroSolution case and the K = 65 / K = 130 network cases
PINNED = [c for c, (_, _, K, _, net) in CASES.items() if net == "zero" or K in (65, 130)]
GOLDEN = "noise_table/plain_form.npz"  # under tests/golden/ (a directory of its own: golden_util lists golden/*.npz)


def widths(net):
    return {"mlp128x4": [128] * 4, "mlp64x2": [64] * 2}[net.split("-")[0]]


def equations(kind, nx):
    """(product equation, oracle equation)"""
    if kind == "cha":
        return dpi.Cha(nx, 1.0, 5.0, 1.0), O.Cha(nx, 1.0, 5.0, 1.0)
    eq = dpi.OUProcessEquation(nx=nx, T=1.0, alpha=1.0, num_components=5, mean_scale=1.0, var_scale=2.0,
                               alpha_scale=4.0)
    return eq, O.OUProcessEquation(nx, eq.mean.numpy(), eq.var.numpy(), eq.pi.numpy(), alpha_scale=4.0)


def weights(nx, hidden):
    """[(W, b)] per Linear layer, W in [-2^-k, 2^-k) with k = bit_length(fan_in) // 2, from Philox words."""
    out, sizes = [], [1 + nx] + list(hidden) + [1]
    for layer, (fi, fo) in enumerate(zip(sizes[:-1], sizes[1:])):
        n = fo * fi + fo
        w = np.stack(PH.philox4x32_10(np.arange((n + 3) // 4), layer, nx, 0xD1, 7), axis=-1).reshape(-1)[:n]
        u = (PH.uniform_co(w) - 0.5) * 2.0 ** (1 - fi.bit_length() // 2)
        out.append((u[:fo * fi].reshape(fo, fi).astype(np.float32), u[fo * fi:].astype(np.float32)))
    return out


def nets(net, nx):
    """(product module, oracle net)"""
    if net == "zero":
        return dpi.ZeroSolution(1), O.ZeroNet()
    hidden = widths(net)
    wb = weights(nx, hidden)
    m = dpi.construct_mlp(1 + nx, 1, hidden, ["ELU"] * len(hidden), None)
    lin = [l for l in m if isinstance(l, torch.nn.Linear)]
    with torch.no_grad():
        for l, (W, b) in zip(lin, wb):
            l.weight.copy_(torch.from_numpy(W))
            l.bias.copy_(torch.from_numpy(b))
    onet = O.MLP([W.astype(np.float64) for W, _ in wb], [b.astype(np.float64) for _, b in wb], ["ELU"] * len(hidden))
    return m, onet


def run(case):
    """The labels of one case on the GPU: {"tx", "sample", "generate"} as fp32 numpy arrays (both entry
    points on the same points and counters)."""
    import warnings

    from deeppicarditeration_amd import data as D
    kind, nx, K, M, net = CASES[case]
    eq, _ = equations(kind, nx)
    module, _ = nets(net, nx)
    f32 = net.endswith("-f32")
    L.check(L.load().dpi_set_gemm_precision(L.DPI_GEMM_F32 if f32 else L.DPI_GEMM_AUTO), "gemm precision")
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", D.PartialBlockNote)
            gen = dpi.OnlineDataGenerator(eq, module, 1, 1, device="cuda:0", t_always_uniform=True,
                                          n_estimate_terminal=M, n_estimate_integral=M, n_euler_steps=K, seed=SEED,
                                          epoch=EPOCH, partial_blocks=M % 64 != 0)
        tx, y = gen.sample_with_gradients(N_POINTS)
        y2 = gen.generate_with_gradients(tx, point_base=0)
        torch.cuda.synchronize()
    finally:
        L.check(L.load().dpi_set_gemm_precision(L.DPI_GEMM_AUTO), "gemm precision")
    return {"tx": tx.cpu().numpy(), "sample": y.cpu().numpy(), "generate": y2.cpu().numpy()}


def reference(case, tx):
    """The fp64 oracle's labels at the GPU's points."""
    kind, nx, K, M, net = CASES[case]
    _, oeq = equations(kind, nx)
    _, onet = nets(net, nx)
    return O.labels_grad(oeq, onet, np.asarray(tx, np.float64), M, K, SEED, EPOCH, 0)
