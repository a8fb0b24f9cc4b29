"""The fp64 oracle twin of a gradient-head network (NETWORK.TYPE ValueGradient / OnlyGradient) and the
loader of the head fixtures (tests/golden/heads/*.npz, made by tests/golden/make_golden_heads.py).

The oracle (oracle/dpi_oracle.py) asks a net for `value_grad(tx) -> (u, du/dtx, hdiag)`; a head net
answers from its output columns as the reference's get_f does (picard/data.py:1231-1242):
1 + nx outputs are (u, u_x), nx outputs are u_x with u = 0."""
from pathlib import Path

import numpy as np

from oracle import dpi_oracle as O

HEADS = Path(__file__).resolve().parent / "golden" / "heads"
HEAD_CASES = sorted(p.stem for p in HEADS.glob("*.npz"))


class HeadNet:
    """construct_mlp(1 + nx, n_out, ...) with n_out = 1 + nx or nx; weights (out, in), fp64."""

    def __init__(self, weights, biases, acts):
        self.W = [np.asarray(w, np.float64) for w in weights]
        self.b = [np.asarray(b, np.float64) for b in biases]
        self.acts = list(acts)

    def value_grad(self, tx, need_hdiag=False):
        assert not need_hdiag, "a gradient head has no Hessian"
        nx = tx.shape[1] - 1
        a = tx
        for W, b, act in zip(self.W[:-1], self.b[:-1], self.acts):
            a = O._act(act, a @ W.T + b)[0]
        out = a @ self.W[-1].T + self.b[-1]
        if out.shape[1] == 1 + nx:
            u, ux = out[:, :1], out[:, 1:]
        elif out.shape[1] == nx:
            u, ux = np.zeros((tx.shape[0], 1)), out
        else:
            raise ValueError(out.shape)
        return u, np.concatenate([np.zeros_like(u), ux], axis=1), None  # d/dt is never read


def from_module(module, acts):
    import torch
    lin = [l for l in module if isinstance(l, torch.nn.Linear)]
    return HeadNet([l.weight.detach().double().numpy() for l in lin], [l.bias.detach().double().numpy() for l in lin],
                   acts)


def load(name):
    with np.load(HEADS / f"{name}.npz", allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def fixture_net(f):
    sd = {k[3:]: f[k] for k in f if k.startswith("sd_")}
    idx = sorted({int(k.split(".")[0]) for k in sd})
    return HeadNet([sd[f"{i}.weight"] for i in idx], [sd[f"{i}.bias"] for i in idx], [str(a) for a in f["acts"]])
