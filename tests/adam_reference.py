"""The Adam / AdamW update of the fused fit step (csrc/dpi_fit.h k_fit_wgrad_step) restated in
numpy fp64, in the order of torch's single-tensor Adam (non-capturable):

    Adam with L2 weight decay: g += wd w.        AdamW instead: w *= 1 - lr wd
    m += (g - m)(1 - beta1)
    v = beta2 v + (1 - beta2) g g
    w -= step_size m / (sqrt(v) / bc2_sqrt + eps),  step_size = lr / (1 - beta1^step), bc2_sqrt = sqrt(1 - beta2^step)

tests/test_adam_reference.py holds it to torch.optim.Adam and torch.optim.AdamW in fp64 on the CPU.  No GPU and
no library is needed to import this module."""
import numpy as np


def adam_step(w, m, v, g, step, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=False):
    """One update of one tensor: (w, m, v) after step number `step` (1-based) from the gradient g, as new fp64
    arrays."""
    w, m, v, g = (np.array(a, np.float64) for a in (w, m, v, g))
    b1, b2 = betas
    if weight_decay != 0:
        if decoupled:
            w = w * (1.0 - lr * weight_decay)
        else:
            g = g + weight_decay * w
    m = m + (g - m) * (1.0 - b1)
    v = b2 * v + (1.0 - b2) * g * g
    step_size = lr / (1.0 - b1 ** step)
    bc2_sqrt = np.sqrt(1.0 - b2 ** step)
    w = w - step_size * m / (np.sqrt(v) / bc2_sqrt + eps)
    return w, m, v


def adam_steps(ws, ms, vs, gs, step, **kw):
    """`adam_step` over lists of tensors: (ws, ms, vs) after the step."""
    out = [adam_step(w, m, v, g, step, **kw) for w, m, v, g in zip(ws, ms, vs, gs)]
    return [o[0] for o in out], [o[1] for o in out], [o[2] for o in out]
