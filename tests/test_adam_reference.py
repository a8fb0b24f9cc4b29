"""tests/adam_reference.py against torch.optim.Adam and torch.optim.AdamW in fp64 on the CPU: 5 consecutive steps
from random weights and gradients, weight decay zero and positive; the weights and both moments agree at
rtol 1e-12."""
import numpy as np
import pytest
import torch

import adam_reference as A


@pytest.mark.parametrize("cls, wd", [("Adam", 0.0), ("Adam", 0.01), ("AdamW", 0.0), ("AdamW", 0.01)],
                         ids=["adam", "adam_l2", "adamw_wd0", "adamw"])
def test_reference_is_torchs_single_tensor_adam(cls, wd):
    g = torch.Generator().manual_seed(11)
    shapes = [(5, 3), (5,), (1, 5), (1,)]
    params = [torch.nn.Parameter(torch.randn(s, generator=g, dtype=torch.float64)) for s in shapes]
    kw = dict(lr=3e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
    opt = getattr(torch.optim, cls)(params, foreach=False, **kw)
    ws = [p.detach().numpy().copy() for p in params]
    ms = [np.zeros(s) for s in shapes]
    vs = [np.zeros(s) for s in shapes]
    for step in range(1, 6):
        grads = [torch.randn(s, generator=g, dtype=torch.float64) for s in shapes]
        for p, gr in zip(params, grads):
            p.grad = gr.clone()
        opt.step()
        ws, ms, vs = A.adam_steps(ws, ms, vs, [gr.numpy() for gr in grads], step, decoupled=cls == "AdamW", **kw)
        for p, w, m, v in zip(params, ws, ms, vs):
            st = opt.state[p]
            assert float(st["step"]) == step
            np.testing.assert_allclose(p.detach().numpy(), w, rtol=1e-12, atol=0)
            np.testing.assert_allclose(st["exp_avg"].numpy(), m, rtol=1e-12, atol=0)
            np.testing.assert_allclose(st["exp_avg_sq"].numpy(), v, rtol=1e-12, atol=0)
