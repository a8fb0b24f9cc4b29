"""Networks that carry weight in the label, and the CPU-oracle gate that proves it (no device needed).

The label is g-terms + (T - t) (f(u, grad u) - f_b): the network enters through the second term only,
and at torch's default initialisation that term is 1e-5 .. 1e-2 of the label, so a relative error eps in
a kernel's network phase reaches the asserted rel-L2 as eps x share.  `weighted_mlp` scales a net by
powers of two until the network's and the equation's own terms both carry weight, and `gate` asserts
that with the fp64 oracle (oracle/dpi_oracle.py) alone before anything runs on the GPU:

  share band   rel-L2 between the oracle's labels without the network and with it lies in
               [0.05, 0.95] on every block (value, gradient, Hessian where there is one);
  mutant gate  every structural fault of `mutants` (a unit lost at a tile tail, a wrong column of W1,
               ...) moves the oracle's label by >= 1e-3 rel-L2 on at least one block, 10 x the suite's
               bar of 1e-4 - or by exactly 0.0 on every block, where the equation cannot observe it
               (the output bias with OU, whose f does not read u);
  finiteness   the reference labels are finite.

These are conditions on a test's inputs, not tolerances on the kernel under test."""
import copy

import numpy as np
import torch

import heads_util
from oracle import dpi_oracle as O

SHARE_BAND = (0.05, 0.95)
MUTANT_FLOOR = 1e-3


# ----------------------------------------------------------------------------- nets
def _linears(seq):
    return [l for l in seq if isinstance(l, torch.nn.Linear)]


def _is_pis(module):
    return type(module).__name__ == "PISGradNet"


def oracle_twin(module, oeq=None):
    """The fp64 oracle net of `module`: O.MLP, heads_util.HeadNet for a gradient head, O.PISGradNet
    (which needs the oracle equation `oeq` for g0)."""
    if _is_pis(module):
        return O.PISGradNet({k: v.detach().double().numpy() for k, v in module.state_dict().items()}, oeq,
                            T=float(module.T))
    lin = _linears(module)
    acts = [type(l).__name__ for l in module if not isinstance(l, torch.nn.Linear)]
    if lin[-1].out_features != 1:
        return heads_util.from_module(module, acts)
    return O.MLP([l.weight.detach().double().numpy() for l in lin], [l.bias.detach().double().numpy() for l in lin],
                 acts)


def weighted_mlp(module, hidden_scale, out_scale, oeq=None):
    """Multiply, in place, the hidden-to-hidden Linear weights by hidden_scale and the last Linear's
    weight and bias by out_scale (powers of two: the scaling itself is exact in every number format).
    For PISGradNet only nn_module is scaled; smooth_net, t_encoder and the g0 part stay as
    initialised.  Returns the module and its oracle twin."""
    for s in (hidden_scale, out_scale):
        assert s > 0 and np.log2(s) == int(np.log2(s)), ("scales are powers of two", s)
    lin = _linears(module.nn_module if _is_pis(module) else module)
    with torch.no_grad():
        for l in lin[1:-1]:
            l.weight.mul_(float(hidden_scale))
        lin[-1].weight.mul_(float(out_scale))
        lin[-1].bias.mul_(float(out_scale))
    return module, oracle_twin(module, oeq)


def without_network(onet):
    """The reference point of `share`: ZeroNet, or for PISGradNet the same net with nn_module's last
    layer zeroed (its g0 / smooth part alone is already 0.22 / 0.76 of the label)."""
    if isinstance(onet, O.PISGradNet):
        z = copy.deepcopy(onet)
        W, b = z.nn[-1]
        W[:] = 0.0
        b[:] = 0.0
        return z
    return O.ZeroNet()


# ----------------------------------------------------------------------------- labels, per block
def labels(oeq, onet, tx, M, K, seed, epoch, point_base=0, v=0, delta_t=0.0, hessians=False):
    if hessians:
        return O.labels_grad_hess(oeq, onet, tx, M, K, seed, epoch, point_base)
    return O.labels_grad(oeq, onet, tx, M, K, seed, epoch, point_base, v=v, delta_t=delta_t)


def blocks(y, ref, hess_nx=None):
    """rel-L2 of y against ref per block: value, grad, and hess where the labels carry one (hess_nx: the
    nx of labels laid out value | grad (nx) | Hessian (nx^2))."""
    if hess_nx is None:
        return {"value": O.rel_l2(y[:, :1], ref[:, :1]), "grad": O.rel_l2(y[:, 1:], ref[:, 1:])}
    n = hess_nx
    assert ref.shape[1] == 1 + n + n * n
    return {"value": O.rel_l2(y[:, :1], ref[:, :1]), "grad": O.rel_l2(y[:, 1:1 + n], ref[:, 1:1 + n]),
            "hess": O.rel_l2(y[:, 1 + n:], ref[:, 1 + n:])}


def share(oeq, onet, tx, M, K, seed, epoch, point_base=0, v=0, delta_t=0.0, hessians=False, ref=None):
    """rel-L2, per block, between the oracle's labels without the network (`without_network`) and with it."""
    kw = dict(point_base=point_base, v=v, delta_t=delta_t, hessians=hessians)
    if ref is None:
        ref = labels(oeq, onet, tx, M, K, seed, epoch, **kw)
    return blocks(labels(oeq, without_network(onet), tx, M, K, seed, epoch, **kw), ref, oeq.nx if hessians else None)


# ----------------------------------------------------------------------------- mutants
def _drop_unit(W, b, layer, unit):
    """Hidden unit `unit` of layer `layer` gives act(0) = 0 (ELU and Tanh)."""
    W[layer][unit, :] = 0.0
    b[layer][unit] = 0.0


def _mlp_faults(W, b, head_rows=None):
    """(name, edit) for a stack of Linears W[l] (out, in), b[l]; W[0]'s columns are (t, x)."""
    hidden = [w.shape[0] for w in W[:-1]]
    yield "last_unit_last_layer", lambda W, b: W[-1].__setitem__((slice(None), -1), 0.0)
    yield "last_unit_first_layer", lambda W, b: _drop_unit(W, b, 0, -1)
    if max(hidden) > 16:
        yield "unit_16", lambda W, b: _drop_unit(W, b, int(np.argmax(hidden)), 16)
    yield "last_x_column", lambda W, b: W[0].__setitem__((slice(None), -1), 0.0)
    yield "t_column", lambda W, b: W[0].__setitem__((slice(None), 0), 0.0)
    yield "out_bias", lambda W, b: b[-1].__setitem__(slice(None), 0.0)
    if head_rows is not None:  # a gradient head: rows head_rows.. of the last Linear are grad_x u
        yield "last_grad_row", lambda W, b: _drop_unit(W, b, -1, -1)
        yield "first_grad_row", lambda W, b: _drop_unit(W, b, -1, head_rows)


def mutants(onet):
    """(name, copy of the oracle net with one structural fault of the kind index arithmetic produces)."""
    if isinstance(onet, O.PISGradNet):
        W, b = [w for w, _ in onet.nn], [c for _, c in onet.nn]
        for name, edit in _mlp_faults(W, b):
            if name == "out_bias":
                continue
            m = copy.deepcopy(onet)
            edit([w for w, _ in m.nn], [c for _, c in m.nn])
            yield name, m
        m = copy.deepcopy(onet)  # t_encoder output unit -1
        m.t_enc[-1][0][-1, :] = 0.0
        m.t_enc[-1][1][-1] = 0.0
        yield "t_encoder_last_unit", m
        m = copy.deepcopy(onet)  # smooth_net's last layer, row -1: only its row 0 is read
        m.smooth[-1][0][-1, :] = 0.0
        m.smooth[-1][1][-1] = 0.0
        yield "smooth_last_row", m
        m = copy.deepcopy(onet)  # a hidden unit of smooth_net
        m.smooth[-2][0][-1, :] = 0.0
        m.smooth[-2][1][-1] = 0.0
        yield "smooth_last_hidden_unit", m
        return
    head_rows = None
    if isinstance(onet, heads_util.HeadNet):
        nx = onet.W[0].shape[1] - 1
        head_rows = 1 if onet.W[-1].shape[0] == 1 + nx else 0
    for name, edit in _mlp_faults(onet.W, onet.b, head_rows):
        m = copy.deepcopy(onet)
        edit(m.W, m.b)
        yield name, m


# ----------------------------------------------------------------------------- the gate
def gate(oeq, onet, tx, M, K, seed, epoch, point_base=0, v=0, delta_t=0.0, hessians=False, info=None,
         with_mutants=True):
    """The oracle's reference labels for (oeq, onet, tx), after asserting on the CPU that the case is
    sensitive to its network phase: share band, mutant gate, finiteness (module docstring).  `info`, a
    dict, receives the shares and every mutant's effect.  with_mutants=False leaves the mutant gate to
    tests/test_net_weight_gates.py (the GPU tests: their points are the same to 2e-5, and the mutants
    cost seven more oracle calls per case)."""
    tx = np.asarray(tx, np.float64)
    kw = dict(point_base=point_base, v=v, delta_t=delta_t, hessians=hessians)
    ref = labels(oeq, onet, tx, M, K, seed, epoch, **kw)
    hess_nx = oeq.nx if hessians else None
    assert np.isfinite(ref).all(), "the reference labels are not finite"
    sh = share(oeq, onet, tx, M, K, seed, epoch, ref=ref, **kw)
    effects, exempt = {}, []
    for name, m in mutants(onet) if with_mutants else ():
        e = blocks(labels(oeq, m, tx, M, K, seed, epoch, **kw), ref, hess_nx)
        effects[name] = e
        if all(x == 0.0 for x in e.values()):
            exempt.append(name)  # the equation cannot observe it: shown, not assumed
    if info is not None:
        info.update(share=sh, mutants=effects, exempt=exempt, max_label=float(np.abs(ref).max()))
    lo, hi = SHARE_BAND
    assert all(lo <= s <= hi for s in sh.values()), ("share of the network outside [0.05, 0.95]", sh)
    weak = {k: e for k, e in effects.items() if k not in exempt and max(e.values()) < MUTANT_FLOOR}
    assert not weak, ("mutants that move the label by less than 1e-3 on every block", weak)
    return ref
