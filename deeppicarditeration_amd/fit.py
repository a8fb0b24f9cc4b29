"""The outer fit's objectives — what the reference's solution wrappers compute per training batch
(SURVEY.md §8f rank 3).  PyTorch-ROCm by default (TRAIN.BACKEND: torch); under TRAIN.BACKEND: hip the
loss and the parameter gradients of the value and gradient kinds come from the HIP kernels of
csrc/dpi_fit.h (`device_objective`): in two launches for a construct_mlp value network;
for a PISGradNet, nn_module and its double backward in three launches (`_PISCore`) between the time networks
and the loss, which stay torch's — or, under TRAIN.CORE_FORM: layers, in one launch per layer and pass
(csrc/dpi_fit_layers.h); under TRAIN.PIS_SHELL: hip the time networks, the g0 part and the loss come from HIP as
well (`_PISShell`, csrc/dpi_fit_shell.h).  The fit consumes the device-resident labels.

- `value_objective`: PicardBaseSolution.training_step (picard/solution.py:74-81), the exp(beta t)
  weighted value loss;
- `gradient_objective`: PicardSolutionGradientWrapper.training_step (picard/solution_jac.py:167-213)
  for a value network (output_dim 1): value loss plus the per-dimension gradient losses, combined
  by a loss scaler;
- `head_gradient_objective`: the same training_step for a network that outputs the gradient
  (solution_jac.py:184-194): ValueGradient (output_dim 1 + nx: value and gradient losses from the
  output columns, optionally the aux loss tying the value column's own gradient to the gradient
  columns) and OnlyGradient (output_dim nx: the value loss is 0);
- `gradient_hessian_objective`: PicardSolutionGradientHessianWrapper.training_step
  (solution_jac.py:219-259), plus the Hessian losses (all nx^2 entries, or NUM_HESS_SAMPLES of them
  drawn with `random.sample` as there);
- the loss scalers of solution_jac.py:13-109 and LossFnLinearClip (solution.py:22-33);
- `device_objective`: `value_objective` and `gradient_objective` (FixedLossScaler) on the device, for
  construct_mlp value networks and for PISGradNet;
- `device_step` / `fused_train_steps`: under TRAIN.FUSED_STEP the whole training step of a construct_mlp
  value network (loss, gradients and the Adam / AdamW update) in the same two launches, dpi_fit_step;
- `build_objective`: the wrapper choice of PicardRunner.get_solution (picard_iteration.py:113-118)
  and PicardSolutionGradientWrapper.construct_solution / __init__ (solution_jac.py:112-136).

Each objective is `f(net, tx, y) -> (loss (1,), info dict)`; `net` maps tx (B, 1+nx) -> (B, 1), or
(B, 1+nx) / (B, nx) for the head objectives.
"""
import random

import torch


class LossFnLinearClip(torch.nn.Module):
    """solution.py:22-33: x^2 inside |x| < clip, continued linearly (C^1) outside."""

    def __init__(self, clip: float):
        super().__init__()
        self.clip = torch.scalar_tensor(clip)

    def forward(self, x):
        c = self.clip.to(x)
        return torch.where(torch.abs(x) < c, torch.square(x), 2 * c * torch.abs(x) - c ** 2)


def make_loss_fn(fn_cfg):
    """TRAIN.LOSS.FN (solution.py:62-68): None -> square, otherwise LossFnLinearClip(kwargs.clip)."""
    if fn_cfg is None or fn_cfg.get("cls") is None:
        return torch.square
    return LossFnLinearClip(float(fn_cfg["kwargs"]["clip"]))


class LossScaler:
    """solution_jac.py:13-36.  `scale` combines (v_loss (1,), g_loss (nx,)); `scale_g_h` also
    h_loss (nx^2 or NUM_HESS_SAMPLES,).  Both return (total (1,), info)."""

    registry = {}

    def __init_subclass__(cls, **kw):
        super().__init_subclass__(**kw)
        LossScaler.registry[cls.__name__] = cls

    @classmethod
    def get_class(cls, name):
        try:
            return cls.registry[name]
        except KeyError:
            raise ValueError(f"unknown loss scaler {name!r} (known: {sorted(cls.registry)})") from None

    def scale(self, v_loss, g_loss_multi_dim):
        raise NotImplementedError(f"{type(self).__name__} does not scale value + gradient losses")

    def scale_g_h(self, v_loss, g_loss_multi_dim, h_loss_multi_dim):
        raise NotImplementedError(f"{type(self).__name__} does not scale value + gradient + Hessian losses")


class SimpleLossScaler(LossScaler):
    """solution_jac.py:39-50: one weight a = clamp(v / sum g, 0, 1e3).  As there, the summed
    gradient loss is formed under no_grad too, so it adds to the reported loss but not to the
    parameter gradient (kept for parity; tests/golden/fit_grad_clip_simple.npz pins it)."""

    def scale(self, v_loss, g_loss_multi_dim):
        with torch.no_grad():
            g_loss = torch.sum(g_loss_multi_dim, keepdim=True, dim=-1)
            a = torch.clamp(v_loss / g_loss, min=0.0, max=1e3)
        return v_loss + a * g_loss, {"train_gradient_loss(unscaled)": g_loss, "train_gradient_loss_scaling_factor": a}


class DimensionLossScaler(LossScaler):
    """solution_jac.py:53-68: a weight per dimension, a_d = clamp(v / g_d, 0, 1e3)."""

    def scale(self, v_loss, g_loss_multi_dim):
        with torch.no_grad():
            a = torch.clamp(v_loss / g_loss_multi_dim, min=0.0, max=1e3)
            mean_a = torch.mean(a, dim=0)
        g_loss = torch.sum(a * g_loss_multi_dim, keepdim=True, dim=-1)
        return v_loss + g_loss, {"train_gradient_loss(unscaled)": g_loss, "train_gradient_loss_scaling_factor": mean_a}


class FixedLossScaler(LossScaler):
    """solution_jac.py:71-82."""

    def __init__(self, fixed_weight: float):
        self.fixed_weight = fixed_weight

    def scale(self, v_loss, g_loss_multi_dim):
        g_loss = torch.sum(g_loss_multi_dim, keepdim=True, dim=-1)
        return v_loss + self.fixed_weight * g_loss, {"train_gradient_loss(unscaled)": g_loss}

    def __str__(self):
        return f"FixedLossScaler(fixed_weight={self.fixed_weight})"


class FixedHessianLossScaler(LossScaler):
    """solution_jac.py:85-109."""

    def __init__(self, fixed_gradient_weight: float, fixed_hessian_weight: float):
        self.fixed_gradient_weight = fixed_gradient_weight
        self.fixed_hessian_weight = fixed_hessian_weight

    def scale_g_h(self, v_loss, g_loss_multi_dim, h_loss_multi_dim):
        g_loss = torch.sum(g_loss_multi_dim, keepdim=True, dim=-1)
        h_loss = torch.sum(h_loss_multi_dim, keepdim=True, dim=-1)
        return (v_loss + self.fixed_gradient_weight * g_loss + self.fixed_hessian_weight * h_loss,
                {"train_gradient_loss(unscaled)": g_loss, "train_hessian_loss(unscaled)": h_loss})

    def __str__(self):
        return (f"FixedHessianLossScaler(fixed_gradient_weight={self.fixed_gradient_weight},"
                f" fixed_hessian_weight={self.fixed_hessian_weight})")


def _weight(tx, beta):
    return torch.exp(torch.narrow(tx, -1, 0, 1) * beta)


def _u_and_grad(net, tx, column0=False):
    """u (B, 1) and d u / d tx (B, 1+nx) — the per-row Jacobian of a value network (the reference's
    vmap(jacrev(forward)), solution_jac.py:121), as one reverse pass over the batch sum with the
    graph kept for the parameter gradient.  column0: the network has more outputs and u is its
    column 0 (solution_only_u, solution_jac.py:163-165); the whole output is returned."""
    tx = tx.detach().requires_grad_(True)
    with torch.enable_grad():
        u = net(tx)
        (u_tx,) = torch.autograd.grad((u[:, 0] if column0 else u).sum(), tx, create_graph=True)
    return u, u_tx


def value_objective(beta, loss_fn):
    def objective(net, tx, y):
        loss = torch.mean(_weight(tx, beta) * loss_fn(net(tx) - y[:, :1]), dim=0)
        return loss, {}
    return objective


def gradient_objective(beta, loss_fn, scaler, nx):
    def objective(net, tx, y):
        u, u_tx = _u_and_grad(net, tx)
        w = _weight(tx, beta)
        v_loss = torch.mean(w * loss_fn(u - y[:, :1]), dim=0)
        g_loss = torch.mean(w * loss_fn(u_tx[:, 1:] - y[:, 1:1 + nx]), dim=0)
        loss, info = scaler.scale(v_loss, g_loss)
        info["train_value_loss"] = v_loss
        return loss, info
    return objective


def head_gradient_objective(beta, loss_fn, scaler, nx, output_dim, use_aux_loss=False, weight_aux_loss=0.0):
    """solution_jac.py:184-213 for output_dim nx (OnlyGradient) and 1 + nx (ValueGradient).  The aux
    loss (ValueGradient only) is the unweighted mean of loss_fn(d out[:, 0] / dx - out[:, 1:]), added
    per dimension to the gradient loss with weight_aux_loss."""
    if output_dim not in (nx, 1 + nx) or output_dim == 1:
        raise ValueError(f"head_gradient_objective: output_dim {output_dim} is neither nx = {nx} nor 1 + nx")
    only = output_dim == nx

    def objective(net, tx, y):
        w = _weight(tx, beta)
        info = {}
        if only:
            u_x = net(tx)
            v_loss = torch.zeros(1, device=tx.device, dtype=tx.dtype)
        else:
            if use_aux_loss:
                out, u_tx = _u_and_grad(net, tx, column0=True)
                aux = torch.mean(loss_fn(u_tx[:, 1:] - out[:, 1:]), dim=0)
            else:
                out = net(tx)
            u, u_x = out[:, 0:1], out[:, 1:]
            v_loss = torch.mean(w * loss_fn(u - y[:, :1]), dim=0)
        g_loss = torch.mean(w * loss_fn(u_x - y[:, 1:1 + nx]), dim=0)
        if use_aux_loss and not only:
            g_loss = g_loss + weight_aux_loss * aux
            info["aux_loss"] = aux.mean(dim=-1)
        loss, sinfo = scaler.scale(v_loss, g_loss)
        info.update(sinfo)
        info["train_value_loss"] = v_loss
        return loss, info
    return objective


def gradient_hessian_objective(beta, loss_fn, scaler, nx, num_hess_samples=-1):
    def objective(net, tx, y):
        u, u_tx = _u_and_grad(net, tx)
        w = _weight(tx, beta)
        v_loss = torch.mean(w * loss_fn(u - y[:, :1]), dim=0)
        g_loss = torch.mean(w * loss_fn(u_tx[:, 1:] - y[:, 1:1 + nx]), dim=0)
        hess = torch.func.vmap(torch.func.hessian(lambda z: net(z[None])[0, 0]))(tx)  # (B, 1+nx, 1+nx)
        diff = hess[:, 1:, 1:].reshape(tx.shape[0], nx * nx) - y[:, 1 + nx:1 + nx + nx * nx]
        if num_hess_samples > 0:  # solution_jac.py:246-249 (python's global `random`, as there)
            idx = torch.tensor(random.sample(range(nx * nx), num_hess_samples), dtype=torch.long, device=y.device)
            diff = torch.index_select(diff, 1, idx)
        h_loss = torch.mean(w * loss_fn(diff), dim=0)
        loss, info = scaler.scale_g_h(v_loss, g_loss, h_loss)
        info["train_value_loss"] = v_loss
        return loss, info
    return objective


BACKENDS = ("torch", "hip")  # TRAIN.BACKEND


class _DevicePlan:
    """What `device_objective` needs of one network, checked once: the Linear layers of a
    construct_mlp value network (all-ELU or all-Tanh hidden layers, one output, no NETWORK.BOUND), its
    parameters in state-dict order and the C-ABI shape arguments.  Everything else is refused by name;
    there is no fallback to the torch objectives."""

    def __init__(self, net, nx):
        from . import _lib
        self.net = net
        kind = type(net).__name__
        if kind in ("PicardSolutionEnforceTerminal", "PISGradNet"):  # a PISGradNet takes _PISPlan
            raise NotImplementedError(f"TRAIN.BACKEND: hip with {kind}: the fit kernels take construct_mlp value "
                                      "networks only")
        if not isinstance(net, torch.nn.Sequential):
            raise NotImplementedError(f"TRAIN.BACKEND: hip with a {kind} network: the fit kernels take construct_mlp "
                                      "value networks only")
        mods = list(net)
        if mods and isinstance(mods[-1], torch.nn.Hardtanh):
            raise NotImplementedError("TRAIN.BACKEND: hip with NETWORK.BOUND: the fit kernels have no output clamp")
        lin, acts = mods[0::2], mods[1::2]
        if len(mods) < 3 or len(mods) % 2 == 0 or not all(isinstance(m, torch.nn.Linear) for m in lin):
            raise NotImplementedError("TRAIN.BACKEND: hip: the network is not a construct_mlp Linear / activation chain")
        codes = {torch.nn.ELU: _lib.DPI_ACT_ELU, torch.nn.Tanh: _lib.DPI_ACT_TANH}
        kinds = {type(m) for m in acts}
        if len(kinds) != 1 or next(iter(kinds)) not in codes:
            raise NotImplementedError("TRAIN.BACKEND: hip with NETWORK.ACTIVATIONS "
                                      f"{[type(m).__name__ for m in acts]}: all ELU or all Tanh")
        if any(isinstance(m, torch.nn.ELU) and m.alpha != 1.0 for m in acts):
            raise NotImplementedError("TRAIN.BACKEND: hip with ELU alpha != 1")
        if lin[-1].out_features != 1:
            raise NotImplementedError(f"TRAIN.BACKEND: hip with a network of {lin[-1].out_features} outputs (a gradient "
                                      "head): value networks only")
        if any(m.bias is None for m in lin):
            raise NotImplementedError("TRAIN.BACKEND: hip with a Linear layer without bias")
        if lin[0].in_features != 1 + nx:
            raise ValueError(f"network input width {lin[0].in_features} != 1 + nx = {1 + nx}")
        self.weights = [m.weight for m in lin]
        self.biases = [m.bias for m in lin]
        for p in self.weights + self.biases:
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise NotImplementedError(f"TRAIN.BACKEND: hip with {p.dtype} / non-contiguous parameters: fp32 "
                                          "contiguous parameters only (DATA.FLOAT: float)")
        widths = [m.out_features for m in lin[:-1]]
        if len(widths) > 8 or max(widths) > 256 or nx > 256:
            raise NotImplementedError(f"TRAIN.BACKEND: hip with NETWORK.NEURONS {widths}, nx = {nx}: 1-8 hidden layers "
                                      "of width <= 256 and nx <= 256")
        self.act = codes[next(iter(kinds))]
        self.n_in, self.n_hidden = 1 + nx, len(widths)
        self.widths = (_lib.c_int * len(widths))(*widths)
        self.params = [p for m in lin for p in (m.weight, m.bias)]  # state-dict order
        self.ws = None

    def table(self, tensors):
        from . import _lib
        return (_lib.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _device_batch(plan, tx, y):
    """What both device calls of a construct_mlp fit need of one batch: the loaded library, tx and y as the
    kernels read them, B, the plan's workspace grown to the batch and a fresh `losses` (2 + nx,)."""
    from . import _lib
    lib = _lib.load()
    if tx.device.type != "cuda":
        raise _lib.DPIError("TRAIN.BACKEND: hip needs the batch on the GPU (there is no CPU fallback)")
    if tx.dtype != torch.float32 or y.dtype != torch.float32:
        raise NotImplementedError(f"TRAIN.BACKEND: hip with {tx.dtype} batches: fp32 only (DATA.FLOAT: float)")
    tx, y = tx.detach().contiguous(), y.detach()
    if y.stride(-1) != 1:
        y = y.contiguous()
    B = int(tx.shape[0])
    need = int(lib.dpi_fit_workspace_bytes(plan.n_in, plan.n_hidden, plan.widths, B))
    if plan.ws is None or plan.ws.numel() < need or plan.ws.device != tx.device:
        plan.ws = torch.empty(max(need, 1), dtype=torch.uint8, device=tx.device)
    return lib, tx, y, B, torch.empty(1 + plan.n_in, dtype=torch.float32, device=tx.device)


class _DeviceFit(torch.autograd.Function):
    """losses (2 + nx,) = (total, v_loss, g_loss[nx]) of one batch from dpi_fit_gradients, launched on
    torch's current stream; the parameter gradients it computed are kept and handed to the parameters
    in backward, scaled by the gradient arriving at losses[0]."""

    @staticmethod
    def forward(ctx, plan, tx, y, beta, loss_kind, clip, c, *params):
        from . import _lib
        lib, tx, y, B, losses = _device_batch(plan, tx, y)
        grads = [torch.empty_like(p) for p in params]
        _lib.check(lib.dpi_fit_gradients(plan.n_in, plan.n_hidden, plan.widths, plan.act, plan.table(params[0::2]),
                                         plan.table(params[1::2]), plan.table(grads[0::2]), plan.table(grads[1::2]),
                                         tx.data_ptr(), y.data_ptr(), int(y.stride(0)), B, float(beta), loss_kind,
                                         float(clip), float(c), losses.data_ptr(), plan.ws.data_ptr(), plan.ws.numel(),
                                         torch.cuda.current_stream(tx.device).cuda_stream), "dpi_fit_gradients")
        ctx.grads = grads
        total, parts = losses[:1], losses[1:]
        ctx.mark_non_differentiable(parts)
        return total, parts

    @staticmethod
    def backward(ctx, g_total, _g_parts):
        return (None,) * 7 + tuple(torch._foreach_mul(ctx.grads, g_total.reshape(())))


PIS_CHANNELS, PIS_LAYERS_MAX, PIS_WIDTH_MAX, PIS_NX_MAX = 64, 4, 512, 128  # csrc/dpi_fit.h CORE_*
# TRAIN.CORE_FORM -> the C entries of the PISGradNet core (workspace bytes, forward, backward): "tiles" is one
# workgroup per 64 rows through all layers (csrc/dpi_fit.h), "layers" one launch per layer and pass over
# (row tile x unit block) (csrc/dpi_fit_layers.h).  Same primitive, contract and workspace arrays.
CORE_FORMS = {"tiles": ("dpi_fit_core_workspace_bytes", "dpi_fit_core_forward", "dpi_fit_core_backward"),
              "layers": ("dpi_fit_core_layers_workspace_bytes", "dpi_fit_core_layers_forward",
                         "dpi_fit_core_layers_backward")}


def _check_core_form(core_form):
    if core_form not in CORE_FORMS:
        raise ValueError(f"TRAIN.CORE_FORM {core_form!r}: one of {tuple(CORE_FORMS)}")


# TRAIN.PIS_SHELL: what computes a PISGradNet's objective around the core.  "torch": the time networks and the loss
# are torch ops under autograd (`_pis_objective`); "hip": the C entries dpi_fit_shell_* (csrc/dpi_fit_shell.h),
# chained with the core's in `_PISShell`.
PIS_SHELLS = ("torch", "hip")


def _check_pis_shell(pis_shell):
    if pis_shell not in PIS_SHELLS:
        raise ValueError(f"TRAIN.PIS_SHELL {pis_shell!r}: one of {PIS_SHELLS}")


def _refuse_shell_without_pisgradnet(pis_shell, net):
    if pis_shell != "torch" and type(net).__name__ != "PISGradNet":
        raise NotImplementedError(f"TRAIN.PIS_SHELL: {pis_shell} with a {type(net).__name__} network: the shell is a "
                                  "PISGradNet's (NETWORK.PISGRADNET)")


class _PISPlan:
    """What `device_objective` needs of one PISGradNet (this build's class or the reference's of that
    name), checked once and before the library is touched: the closed-form g and g_x behind g0, the
    Linear layers of `nn_module` (the part the HIP core computes), its parameters in state-dict order
    and the C-ABI shape arguments.  What the core does not cover is refused by name.  core_form
    (TRAIN.CORE_FORM) names the C entries `_PISCore` calls."""

    def __init__(self, net, nx, core_form="tiles", pis_shell="torch"):
        from . import _lib
        _check_core_form(core_form)
        _check_pis_shell(pis_shell)
        self.net = net
        self.core_form = core_form
        self.pis_shell = pis_shell
        self.ws_bytes, self.forward, self.backward = CORE_FORMS[core_form]
        owner = getattr(net.g0, "__self__", None)
        if owner is None or type(owner).__name__ != "OUProcessEquation":
            raise NotImplementedError("TRAIN.BACKEND: hip with a PISGradNet whose g0 is not the bound method g of an "
                                      "OUProcessEquation: the device fit needs the closed-form gradient g_x of g0")
        self.equation = owner
        if net.channels != PIS_CHANNELS:
            raise NotImplementedError(f"TRAIN.BACKEND: hip with PISGradNet channels = {net.channels}: the core kernels "
                                      f"take {PIS_CHANNELS} time channels")
        if net.dim != nx:
            raise ValueError(f"PISGradNet dim {net.dim} != nx = {nx}")
        mods = list(net.nn_module)
        lin, acts = mods[0::2], mods[1::2]
        if (len(mods) < 3 or len(mods) % 2 == 0 or not all(isinstance(m, torch.nn.Linear) and m.bias is not None
                                                           for m in lin)
                or not all(isinstance(m, torch.nn.ELU) and m.alpha == 1.0 for m in acts)):
            raise NotImplementedError("TRAIN.BACKEND: hip with a PISGradNet whose nn_module is not a Linear / ELU "
                                      "(alpha = 1) chain with biases")
        widths = [m.out_features for m in lin[:-1]]
        if len(widths) > PIS_LAYERS_MAX or max(widths) > PIS_WIDTH_MAX:
            raise NotImplementedError(f"TRAIN.BACKEND: hip with PISGradNet NETWORK.NEURONS {widths}: 1-"
                                      f"{PIS_LAYERS_MAX} hidden layers of width <= {PIS_WIDTH_MAX}")
        if nx > PIS_NX_MAX:
            raise NotImplementedError(f"TRAIN.BACKEND: hip with PISGradNet at nx = {nx}: nx <= {PIS_NX_MAX}")
        if lin[0].in_features != PIS_CHANNELS + nx or lin[-1].out_features != nx:
            raise ValueError(f"PISGradNet nn_module maps {lin[0].in_features} -> {lin[-1].out_features}, not "
                             f"{PIS_CHANNELS} + nx -> nx")
        for p in net.parameters():
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise NotImplementedError(f"TRAIN.BACKEND: hip with PISGradNet and {p.dtype} / non-contiguous "
                                          "parameters: fp32 contiguous parameters only (DATA.FLOAT: float)")
        self.nx, self.n_hidden = nx, len(widths)
        self.widths = (_lib.c_int * len(widths))(*widths)
        self.params = [p for m in lin for p in (m.weight, m.bias)]  # state-dict order
        self.ws = None
        self.calls = 0  # forward calls so far: a backward must find the state of its own forward in ws
        if pis_shell == "hip":
            self._shell_table(owner)

    def _shell_table(self, equation):
        """TRAIN.PIS_SHELL: hip: the time networks' parameters in state-dict order (the table of dpi_fit_shell_*),
        the timestep_coeff buffer and the equation that hands out the problem handle; the shell has a workspace of
        its own."""
        net, nx = self.net, self.nx
        if not callable(getattr(equation, "dpi_problem", None)):
            raise NotImplementedError(f"TRAIN.PIS_SHELL: hip with a {type(equation).__name__} that has no dpi_problem(): "
                                      "the shell kernels take g0 from the compiled problem handle")
        chains = []
        for name, seq, dims in (("t_encoder", net.t_encoder, [2 * PIS_CHANNELS, PIS_CHANNELS, PIS_CHANNELS]),
                                ("smooth_net", net.smooth_net,
                                 [2 * PIS_CHANNELS] + [PIS_CHANNELS] * (self.n_hidden + 1) + [nx])):
            mods = list(seq)
            lin, acts = mods[0::2], mods[1::2]
            if (len(mods) != 2 * len(dims) - 3 or not all(isinstance(m, torch.nn.Linear) and m.bias is not None
                                                          for m in lin)
                    or not all(isinstance(m, torch.nn.ELU) and m.alpha == 1.0 for m in acts)
                    or [(m.in_features, m.out_features) for m in lin] != list(zip(dims[:-1], dims[1:]))):
                raise NotImplementedError(f"TRAIN.PIS_SHELL: hip with a PISGradNet whose {name} is not the Linear / ELU "
                                          f"(alpha = 1) chain {' -> '.join(map(str, dims))} with biases")
            chains += [p for m in lin for p in (m.weight, m.bias)]
        coeff = net.timestep_coeff
        if coeff.dtype != torch.float32 or not coeff.is_contiguous() or coeff.numel() != PIS_CHANNELS:
            raise NotImplementedError("TRAIN.PIS_SHELL: hip with a timestep_coeff buffer that is not fp32 contiguous of "
                                      f"{PIS_CHANNELS} entries")
        self.shell_equation = equation
        self.shell_params = [net.timestep_phase] + chains
        self.shell_ws = None

    def table(self, tensors):
        from . import _lib
        return (_lib.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


class _PISCore(torch.autograd.Function):
    """PISGradNet's nn_module N as one differentiable primitive: (tau (B, 64), x (B, nx),
    *params) -> sp = x . N(tau, x) (B, 1) and q = d sp / d x (B, nx), from dpi_fit_core_forward; backward
    is dpi_fit_core_backward (the gradients of tau and of the parameters; x is data and gets none), so
    no torch double backward is involved.  grad False: only sp is formed, q is empty.  Under
    TRAIN.CORE_FORM: layers the plan names dpi_fit_core_layers_forward / _backward instead."""

    @staticmethod
    def forward(ctx, plan, grad, tau, x, *params):
        from . import _lib
        lib = _lib.load()
        tau, x = tau.detach(), x.detach()
        if tau.stride(-1) != 1:
            tau = tau.contiguous()
        if x.stride(-1) != 1:
            x = x.contiguous()
        B, nx = int(x.shape[0]), plan.nx
        need = int(getattr(lib, plan.ws_bytes)(nx, plan.n_hidden, plan.widths, B))
        if plan.ws is None or plan.ws.numel() < need or plan.ws.device != x.device:
            plan.ws = torch.empty(max(need, 4), dtype=torch.uint8, device=x.device)
        sp = torch.empty(B, 1, dtype=torch.float32, device=x.device)
        q = torch.empty(B if grad else 0, nx, dtype=torch.float32, device=x.device)
        _lib.check(getattr(lib, plan.forward)(nx, plan.n_hidden, plan.widths, plan.table(params[0::2]),
                                              plan.table(params[1::2]), tau.data_ptr(), int(tau.stride(0)),
                                              x.data_ptr(), int(x.stride(0)), B, sp.data_ptr(),
                                              q.data_ptr() if grad else None, plan.ws.data_ptr(), plan.ws.numel(),
                                              torch.cuda.current_stream(x.device).cuda_stream), plan.forward)
        plan.calls += 1
        ctx.plan, ctx.grad, ctx.call, ctx.params, ctx.B = plan, grad, plan.calls, params, B
        if not grad:
            ctx.mark_non_differentiable(q)
        return sp, q

    @staticmethod
    def backward(ctx, g_sp, g_q):
        from . import _lib
        lib = _lib.load()
        plan, params, B = ctx.plan, ctx.params, ctx.B
        if plan.calls != ctx.call:
            raise RuntimeError("the PISGradNet core's state was overwritten by a later forward call on the same "
                               "network before this backward ran")
        dev = plan.ws.device
        e = (torch.zeros(B, 1, dtype=torch.float32, device=dev) if g_sp is None else g_sp.float().contiguous())
        r = g_q.float().contiguous() if ctx.grad and g_q is not None else None
        grads = [torch.empty_like(p) for p in params]
        dtau = torch.empty(B, PIS_CHANNELS, dtype=torch.float32, device=dev)
        _lib.check(getattr(lib, plan.backward)(plan.nx, plan.n_hidden, plan.widths, plan.table(params[0::2]),
                                               plan.table(params[1::2]), plan.table(grads[0::2]),
                                               plan.table(grads[1::2]), e.data_ptr(),
                                               None if r is None else r.data_ptr(), B, dtau.data_ptr(),
                                               plan.ws.data_ptr(), plan.ws.numel(),
                                               torch.cuda.current_stream(dev).cuda_stream), plan.backward)
        return (None, None, dtau, None) + tuple(grads)


class _PISShell(torch.autograd.Function):
    """A PISGradNet's whole objective from the library (TRAIN.PIS_SHELL: hip): losses (2 + nx,) =
    (total, v_loss, g_loss[nx]) of one batch.  Its forward chains dpi_fit_shell_forward (tau, s, the g0 part), the
    core's forward of the plan's form (sp, q), dpi_fit_shell_loss (the loss and the seeds e, r, sbar), the core's
    backward (nn_module's gradients and taubar) and dpi_fit_shell_backward (the time networks' gradients) on
    torch's current stream, with no host synchronisation; the gradients are kept and handed to the parameters
    in backward, scaled by the gradient arriving at losses[0], as `_DeviceFit` does.  params: the shell's table,
    then nn_module's."""

    @staticmethod
    def forward(ctx, plan, tx, y, beta, loss_kind, clip, kappa, *params):
        from . import _lib
        lib = _lib.load()
        tx, y = tx.detach(), y.detach()
        if tx.stride(-1) != 1:
            tx = tx.contiguous()
        if y.stride(-1) != 1:
            y = y.contiguous()
        B, nx, dev = int(tx.shape[0]), plan.nx, tx.device
        grad = kappa > 1e-9
        ns = len(plan.shell_params)
        shell_p, core_p = params[:ns], params[ns:]
        need = int(lib.dpi_fit_shell_workspace_bytes(nx, plan.n_hidden, B))
        if plan.shell_ws is None or plan.shell_ws.numel() < need or plan.shell_ws.device != dev:
            plan.shell_ws = torch.empty(max(need, 8), dtype=torch.uint8, device=dev)
        need = int(getattr(lib, plan.ws_bytes)(nx, plan.n_hidden, plan.widths, B))
        if plan.ws is None or plan.ws.numel() < need or plan.ws.device != dev:
            plan.ws = torch.empty(max(need, 4), dtype=torch.uint8, device=dev)
        sws, cws = plan.shell_ws, plan.ws
        st = torch.cuda.current_stream(dev).cuda_stream
        new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)  # noqa: E731
        ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        W, b = plan.table(core_p[0::2]), plan.table(core_p[1::2])
        tau, s, res, sp = new(B, PIS_CHANNELS), new(B), new(B), new(B)
        res_x, q, r = (new(B, nx), new(B, nx), new(B, nx)) if grad else (None, None, None)
        _lib.check(lib.dpi_fit_shell_forward(plan.shell_equation.dpi_problem(), float(plan.net.T), nx, plan.n_hidden,
                                             plan.net.timestep_coeff.data_ptr(), plan.table(shell_p), tx.data_ptr(),
                                             int(tx.stride(0)), B, int(grad), tau.data_ptr(), s.data_ptr(),
                                             res.data_ptr(), ptr(res_x), sws.data_ptr(), sws.numel(), st),
                   "dpi_fit_shell_forward")
        # x is the columns 1 .. nx of tx, read in place through its row stride
        _lib.check(getattr(lib, plan.forward)(nx, plan.n_hidden, plan.widths, W, b, tau.data_ptr(), PIS_CHANNELS,
                                              tx.data_ptr() + tx.element_size(), int(tx.stride(0)), B, sp.data_ptr(),
                                              ptr(q), cws.data_ptr(), cws.numel(), st), plan.forward)
        losses, e, sbar = new(2 + nx), new(B), new(B)
        _lib.check(lib.dpi_fit_shell_loss(nx, sp.data_ptr(), ptr(q), s.data_ptr(), res.data_ptr(), ptr(res_x),
                                          tx.data_ptr(), int(tx.stride(0)), y.data_ptr(), int(y.stride(0)), B,
                                          float(beta), loss_kind, float(clip), float(kappa), losses.data_ptr(),
                                          e.data_ptr(), ptr(r), sbar.data_ptr(), sws.data_ptr(), sws.numel(), st),
                   "dpi_fit_shell_loss")
        core_g, shell_g = [torch.empty_like(p) for p in core_p], [torch.empty_like(p) for p in shell_p]
        dtau = new(B, PIS_CHANNELS)
        _lib.check(getattr(lib, plan.backward)(nx, plan.n_hidden, plan.widths, W, b, plan.table(core_g[0::2]),
                                               plan.table(core_g[1::2]), e.data_ptr(), ptr(r), B, dtau.data_ptr(),
                                               cws.data_ptr(), cws.numel(), st), plan.backward)
        _lib.check(lib.dpi_fit_shell_backward(nx, plan.n_hidden, plan.table(shell_p), plan.table(shell_g),
                                              dtau.data_ptr(), sbar.data_ptr(), B, sws.data_ptr(), sws.numel(), st),
                   "dpi_fit_shell_backward")
        plan.calls += 1
        ctx.grads = shell_g + core_g
        total, parts = losses[:1], losses[1:]
        ctx.mark_non_differentiable(parts)
        return total, parts

    @staticmethod
    def backward(ctx, g_total, _g_parts):
        return (None,) * 7 + tuple(torch._foreach_mul(ctx.grads, g_total.reshape(())))


def _pis_shell_objective(plan, tx, y, beta, loss_kind, clip, kappa, value_only):
    """`_pis_objective` with the shell in HIP: the same loss shape and `info` keys from `_PISShell`'s losses."""
    from . import _lib
    if tx.dtype != torch.float32 or y.dtype != torch.float32:
        raise NotImplementedError(f"TRAIN.BACKEND: hip with PISGradNet and {tx.dtype} batches: fp32 only "
                                  "(DATA.FLOAT: float)")
    if tx.device.type != "cuda":
        raise _lib.DPIError("TRAIN.BACKEND: hip needs the batch on the GPU (there is no CPU fallback)")
    total, parts = _PISShell.apply(plan, tx, y, beta, loss_kind, clip, 0.0 if value_only else kappa,
                                   *plan.shell_params, *plan.params)
    if value_only:
        return total, {}
    return total, {"train_gradient_loss(unscaled)": parts[1:].sum(dim=-1, keepdim=True), "train_value_loss": parts[:1]}


def _pis_objective(plan, tx, y, beta, loss_fn, scaler, value_only):
    """`value_objective` / `gradient_objective` on a PISGradNet u = s sp + (1 - s) g0(c x): the time
    networks (t_encoder, smooth_net, the embedding) run in torch with ordinary autograd, the parameter-free
    g0 part under no_grad from the equation's closed forms, sp and q = d sp / d x come from `_PISCore`, and
    the loss is formed in torch ops."""
    from . import _lib
    if tx.dtype != torch.float32 or y.dtype != torch.float32:
        raise NotImplementedError(f"TRAIN.BACKEND: hip with PISGradNet and {tx.dtype} batches: fp32 only "
                                  "(DATA.FLOAT: float)")
    if tx.device.type != "cuda":
        raise _lib.DPIError("TRAIN.BACKEND: hip needs the batch on the GPU (there is no CPU fallback)")
    net, nx = plan.net, plan.nx
    tx = tx.detach()
    t, x = torch.narrow(tx, -1, 0, 1), torch.narrow(tx, -1, 1, nx)
    lbd = net.T - t
    s = net.smoothing_function(lbd)
    tau = net.t_encoder(net.get_pis_timestep_embedding(lbd))
    with torch.no_grad():
        cf = torch.exp(-0.5 * lbd)
        res = plan.equation.g(cf * x)
        res_x = None if value_only else cf * plan.equation.g_x(cf * x)
    sp, q = _PISCore.apply(plan, not value_only, tau, x, *plan.params)
    w = _weight(tx, beta)
    u = s * sp + (1.0 - s) * res
    v_loss = torch.mean(w * loss_fn(u - y[:, :1]), dim=0)
    if value_only:
        return v_loss, {}
    u_x = s * q + (1.0 - s) * res_x
    g_loss = torch.mean(w * loss_fn(u_x - y[:, 1:1 + nx]), dim=0)
    loss, info = scaler.scale(v_loss, g_loss)
    info["train_value_loss"] = v_loss
    return loss, info


def _device_loss_args(loss_fn, scaler):
    """(loss_kind, clip, c, value_only) of the C calls from the loss function and the scaler; what the kernels
    do not have is refused by name."""
    from . import _lib
    if scaler is not None and not isinstance(scaler, FixedLossScaler):
        raise NotImplementedError(f"TRAIN.BACKEND: hip with {type(scaler).__name__}: FixedLossScaler only")
    if isinstance(loss_fn, LossFnLinearClip):
        loss_kind, clip = _lib.DPI_FIT_LOSS_CLIP, float(loss_fn.clip)
    elif loss_fn is torch.square:
        loss_kind, clip = _lib.DPI_FIT_LOSS_SQUARE, 0.0
    else:
        raise NotImplementedError(f"TRAIN.BACKEND: hip with the loss function {loss_fn!r}: the square or LossFnLinearClip")
    c = 0.0 if scaler is None else float(scaler.fixed_weight)
    return loss_kind, clip, c, c <= 1e-9


def device_objective(beta, loss_fn, scaler, nx, core_form="tiles", pis_shell="torch"):
    """The device form of `value_objective` (scaler None, or a FixedLossScaler of weight <= 1e-9) and of
    `gradient_objective` with a FixedLossScaler: loss and parameter gradients from the HIP kernels of
    csrc/dpi_fit.h, same signature and `info` keys.  The optimizer stays torch's:
    `loss.sum().backward()` delivers the gradients the forward launch computed.  The network decides at
    the first batch: a construct_mlp value network takes `_DeviceFit` (loss and gradients in two launches),
    a PISGradNet takes `_pis_objective` (nn_module in HIP through `_PISCore`, the rest in torch).
    core_form (TRAIN.CORE_FORM): the form of the PISGradNet core, "tiles" or "layers"; "layers" with any other
    network is refused by name at the first batch, before the library is touched.
    pis_shell (TRAIN.PIS_SHELL): "torch", or "hip": a PISGradNet's whole objective from the library (`_PISShell`:
    the time networks, the g0 part, the loss and every parameter gradient in HIP, with either form of the core);
    "hip" with any other network is refused the same way."""
    _check_core_form(core_form)
    _check_pis_shell(pis_shell)
    loss_kind, clip, c, value_only = _device_loss_args(loss_fn, scaler)
    plans = {}

    def objective(net, tx, y):
        plan = plans.get(id(net))
        if plan is None or plan.net is not net:
            _refuse_shell_without_pisgradnet(pis_shell, net)
            if type(net).__name__ == "PISGradNet":
                shell = () if pis_shell == "torch" else (pis_shell,)  # the default reproduces the call as it was
                plan = plans[id(net)] = _PISPlan(net, nx, core_form, *shell)
            elif core_form != "tiles":
                raise NotImplementedError(f"TRAIN.CORE_FORM: {core_form} with a {type(net).__name__} network: the "
                                          "forms are the PISGradNet core's (NETWORK.PISGRADNET)")
            else:
                plan = plans[id(net)] = _DevicePlan(net, nx)
        if isinstance(plan, _PISPlan):
            if plan.pis_shell == "hip":
                return _pis_shell_objective(plan, tx, y, beta, loss_kind, clip, c, value_only)
            return _pis_objective(plan, tx, y, beta, loss_fn, scaler, value_only)
        total, parts = _DeviceFit.apply(plan, tx, y, beta, loss_kind, clip, 0.0 if value_only else c, *plan.params)
        if value_only:
            return total, {}
        return total, {"train_gradient_loss(unscaled)": parts[1:].sum(dim=-1, keepdim=True),
                       "train_value_loss": parts[:1]}
    return objective


FUSED_OPTIMIZERS = ("Adam", "AdamW")  # TRAIN.FUSED_STEP: the updates k_fit_wgrad_step applies


def _fused_group(opt, plan):
    """The single param group of `opt` as the fused step reads it on every step, checked: torch.optim.Adam
    or AdamW itself over exactly the plan's parameters, in torch's plain single-tensor arithmetic."""
    if type(opt) not in (torch.optim.Adam, torch.optim.AdamW):
        raise NotImplementedError(f"TRAIN.FUSED_STEP with TRAIN.OPTIMIZER.cls {type(opt).__name__}: "
                                  f"{' or '.join(FUSED_OPTIMIZERS)} only")
    if len(opt.param_groups) != 1:
        raise NotImplementedError(f"TRAIN.FUSED_STEP with {len(opt.param_groups)} param groups: one param group only")
    group = opt.param_groups[0]
    for key in ("amsgrad", "maximize", "capturable", "differentiable", "fused"):
        if group.get(key):
            raise NotImplementedError(f"TRAIN.FUSED_STEP with TRAIN.OPTIMIZER.kwargs {key}: the fused step is torch's "
                                      "plain single-tensor update")
    if isinstance(group["lr"], torch.Tensor) or any(isinstance(b, torch.Tensor) for b in group["betas"]):
        raise NotImplementedError("TRAIN.FUSED_STEP with a tensor lr or tensor betas: the step size is formed on the "
                                  "host from floats")
    if sorted(map(id, group["params"])) != sorted(map(id, plan.params)):
        raise NotImplementedError("TRAIN.FUSED_STEP with a param group that is not exactly the network's parameters")
    return group


def _fused_state(opt, plan):
    """opt.state of every parameter of the plan, created where it is missing the way torch's Adam creates it at
    its first step (`step` a CPU scalar tensor, the moments zeros like the parameter); the step
    counters must agree, as they do after any number of steps of either form."""
    states = []
    for p in plan.params:
        st = opt.state[p]
        if len(st) == 0:
            st["step"] = torch.tensor(0.0, dtype=(torch.float64 if torch.get_default_dtype() == torch.float64
                                                  else torch.float32))
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        for key in ("exp_avg", "exp_avg_sq"):
            m = st[key]
            if m.dtype != torch.float32 or not m.is_contiguous() or m.shape != p.shape or m.device != p.device:
                raise NotImplementedError(f"TRAIN.FUSED_STEP with an optimizer state {key} that is not an fp32 contiguous "
                                          "tensor like its parameter")
        states.append(st)
    if len({float(st["step"]) for st in states}) != 1:
        raise NotImplementedError("TRAIN.FUSED_STEP with parameters at different optimizer step counts")
    return states


def device_step(beta, loss_fn, scaler, nx, core_form="tiles", pis_shell="torch"):
    """One whole training step on the device (TRAIN.FUSED_STEP under TRAIN.BACKEND: hip):
    `step(net, opt, tx, y) -> losses (2 + nx,)` = (total, v_loss, g_loss[nx]) of the batch, formed before the
    update, from dpi_fit_step: k_fit_rows and k_fit_wgrad_step compute the loss and the gradients and apply
    the Adam / AdamW update of every parameter in the same two launches, with no autograd and no gradient
    tensors: `p.grad` stays None.  `opt` is the torch.optim.Adam / AdamW `make_optimizer` builds: lr, betas,
    eps and weight_decay are read from its one param group on every step (so host-side schedulers keep
    working), the moments and the counter live in `opt.state` in torch's layout (so `opt.state_dict()` is
    torch's and a run may switch between the two step forms).  Same options as `device_objective`; an
    optimizer or network the kernel does not cover is refused by name at the first batch, before the library
    is touched.  There is no fallback.  core_form other than "tiles" is refused as `device_objective` refuses
    it: the fused step has no PISGradNet core; so is pis_shell other than "torch"."""
    _check_core_form(core_form)
    _check_pis_shell(pis_shell)
    loss_kind, clip, c, value_only = _device_loss_args(loss_fn, scaler)
    plans = {}

    def step(net, opt, tx, y):
        plan = plans.get(id(net))
        if plan is None or plan.net is not net:
            _refuse_shell_without_pisgradnet(pis_shell, net)
            if core_form != "tiles" and type(net).__name__ != "PISGradNet":
                raise NotImplementedError(f"TRAIN.CORE_FORM: {core_form} with a {type(net).__name__} network: the "
                                          "forms are the PISGradNet core's (NETWORK.PISGRADNET)")
            if type(net).__name__ == "PISGradNet":
                raise NotImplementedError("TRAIN.FUSED_STEP with NETWORK.PISGRADNET (a PISGradNet): its time networks "
                                          "are fitted by torch")
            plan = plans[id(net)] = _DevicePlan(net, nx)
        group = _fused_group(opt, plan)
        states = _fused_state(opt, plan)
        from . import _lib
        lib, tx, y, B, losses = _device_batch(plan, tx, y)
        t = int(states[0]["step"]) + 1
        b1, b2 = group["betas"]
        decoupled = isinstance(opt, torch.optim.AdamW) or bool(group.get("decoupled_weight_decay"))
        m, v = [st["exp_avg"] for st in states], [st["exp_avg_sq"] for st in states]
        _lib.check(lib.dpi_fit_step(plan.n_in, plan.n_hidden, plan.widths, plan.act, plan.table(plan.params[0::2]),
                                    plan.table(plan.params[1::2]), None, None, plan.table(m[0::2]), plan.table(m[1::2]),
                                    plan.table(v[0::2]), plan.table(v[1::2]), tx.data_ptr(), y.data_ptr(),
                                    int(y.stride(0)), B, float(beta), loss_kind, float(clip),
                                    0.0 if value_only else float(c), float(group["lr"]), float(b1), float(b2),
                                    float(group["eps"]), float(group["weight_decay"]), int(decoupled), t,
                                    losses.data_ptr(), plan.ws.data_ptr(), plan.ws.numel(),
                                    torch.cuda.current_stream(tx.device).cuda_stream), "dpi_fit_step")
        for st in states:
            st["step"] += 1
        return losses
    return step


def step_info(losses, value_only=False):
    """The `info` of `device_objective` from the losses (2 + nx,) of one fused step."""
    if value_only:
        return {}
    return {"train_gradient_loss(unscaled)": losses[2:].sum(dim=-1, keepdim=True), "train_value_loss": losses[1:2]}


def make_scaler(scaler_cfg):
    """solution_jac.py:132-136: no SCALER.cls means FixedLossScaler(1.0)."""
    if scaler_cfg is None or scaler_cfg.get("cls") is None:
        return FixedLossScaler(1.0)
    return LossScaler.get_class(scaler_cfg["cls"])(**dict(scaler_cfg.get("kwargs") or {}))


def build_objective(train_cfg, nx, supervise_gradient, supervise_hessian, output_dim=1, backend="torch",
                    fused_step=False, core_form="tiles", pis_shell="torch"):
    """PicardRunner.get_solution (picard_iteration.py:113-118) + the wrappers' construct_solution
    (solution_jac.py:112-119): returns (objective, kind) with kind in {"value", "gradient",
    "gradient_hessian", "head_value_gradient", "head_only_gradient"}.  output_dim: the network's
    output width (1: a Value net; 1 + nx / nx: a ValueGradient / OnlyGradient head).  A
    FixedLossScaler of weight <= 1e-9 falls back to the plain value fit (Value nets).
    backend (TRAIN.BACKEND): "torch" builds the objectives above; "hip" builds `device_objective` for the
    kinds "value" and "gradient" with FixedLossScaler and refuses every other option by name.
    fused_step (TRAIN.FUSED_STEP, "hip" only): what is returned in the objective's place is the `device_step`
    of the same options, for `fused_train_steps`.
    core_form (TRAIN.CORE_FORM, other than "tiles" under "hip" only): handed to `device_objective`.
    pis_shell (TRAIN.PIS_SHELL, "hip" under backend "hip" only): handed on the same way."""
    if backend not in BACKENDS:
        raise ValueError(f"TRAIN.BACKEND {backend!r}: one of {BACKENDS}")
    _check_core_form(core_form)
    _check_pis_shell(pis_shell)
    if pis_shell != "torch" and backend != "hip":
        raise NotImplementedError(f"TRAIN.PIS_SHELL: {pis_shell} with TRAIN.BACKEND: {backend}: the shell kernels are "
                                  "the HIP fit's (TRAIN.BACKEND: hip)")
    if core_form != "tiles" and backend != "hip":
        raise NotImplementedError(f"TRAIN.CORE_FORM: {core_form} with TRAIN.BACKEND: {backend}: the core's forms are "
                                  "the HIP fit's (TRAIN.BACKEND: hip)")
    if fused_step and backend != "hip":
        raise NotImplementedError(f"TRAIN.FUSED_STEP with TRAIN.BACKEND: {backend}: the fused step is the HIP fit's "
                                  "(TRAIN.BACKEND: hip)")
    if backend == "hip":
        return _build_device_objective(train_cfg, nx, supervise_gradient, supervise_hessian, output_dim,
                                       device_step if fused_step else device_objective, core_form, pis_shell)
    loss_cfg = train_cfg["LOSS"]
    beta = float(loss_cfg["beta"])
    loss_fn = make_loss_fn(loss_cfg.get("FN"))
    head = output_dim != 1
    if head and output_dim not in (nx, 1 + nx):
        raise ValueError(f"network output width {output_dim}: must be 1, 1 + nx = {1 + nx} or nx = {nx}")
    if head and supervise_hessian:
        raise NotImplementedError("TRAIN.SUPERVISE_HESSIAN with a ValueGradient / OnlyGradient network: Hessian "
                                  "supervision of a gradient head is out of scope")
    if head and not supervise_gradient:
        raise NotImplementedError("a ValueGradient / OnlyGradient network is fitted to gradient labels: set "
                                  "TRAIN.SUPERVISE_GRADIENT (or use an equation with a gradient term)")
    if not (supervise_gradient or supervise_hessian):
        return value_objective(beta, loss_fn), "value"
    aux = bool(loss_cfg.get("use_aux_loss"))
    if aux and output_dim != 1 + nx:
        raise NotImplementedError("TRAIN.LOSS.use_aux_loss applies to ValueGradient networks only")
    scaler = make_scaler(loss_cfg.get("SCALER"))
    if head:
        if isinstance(scaler, FixedLossScaler) and scaler.fixed_weight <= 1e-9:
            raise NotImplementedError("FixedLossScaler fixed_weight <= 1e-9 with a ValueGradient / OnlyGradient network: "
                                      "the plain value fit it selects has no meaning for a gradient head")
        obj = head_gradient_objective(beta, loss_fn, scaler, nx, output_dim, aux,
                                      float(loss_cfg.get("weight_aux_loss") or 0.0))
        return obj, "head_only_gradient" if output_dim == nx else "head_value_gradient"
    if isinstance(scaler, FixedLossScaler) and scaler.fixed_weight <= 1e-9:
        return value_objective(beta, loss_fn), "value"
    if supervise_hessian:
        n_h = int(train_cfg.get("NUM_HESS_SAMPLES", -1) or -1)
        if n_h > nx * nx:
            raise AssertionError(f"NUM_HESS_SAMPLES {n_h} > nx^2")
        if not isinstance(scaler, FixedHessianLossScaler):
            raise NotImplementedError(f"{scaler} has no scale_g_h: SUPERVISE_HESSIAN needs FixedHessianLossScaler")
        return gradient_hessian_objective(beta, loss_fn, scaler, nx, n_h), "gradient_hessian"
    return gradient_objective(beta, loss_fn, scaler, nx), "gradient"


def _build_device_objective(train_cfg, nx, supervise_gradient, supervise_hessian, output_dim, make,
                            core_form="tiles", pis_shell="torch"):
    """build_objective under TRAIN.BACKEND: hip.  The options the fit kernels do not cover raise
    NotImplementedError naming the option; the network itself is checked at the first batch.
    make: `device_objective`, or `device_step` under TRAIN.FUSED_STEP."""
    form = {} if core_form == "tiles" else {"core_form": core_form}  # the defaults reproduce the calls as they were
    if pis_shell != "torch":
        form["pis_shell"] = pis_shell
    loss_cfg = train_cfg["LOSS"]
    beta = float(loss_cfg["beta"])
    loss_fn = make_loss_fn(loss_cfg.get("FN"))
    if output_dim != 1:
        raise NotImplementedError("TRAIN.BACKEND: hip with NETWORK.TYPE ValueGradient / OnlyGradient (a gradient head "
                                  f"of {output_dim} outputs): value networks only")
    if supervise_hessian:
        raise NotImplementedError("TRAIN.BACKEND: hip with TRAIN.SUPERVISE_HESSIAN: the fit kernels have the value "
                                  "and gradient losses only")
    if not supervise_gradient:
        return make(beta, loss_fn, None, nx, **form), "value"
    if bool(loss_cfg.get("use_aux_loss")):
        raise NotImplementedError("TRAIN.LOSS.use_aux_loss applies to ValueGradient networks only")
    scaler = make_scaler(loss_cfg.get("SCALER"))
    if not isinstance(scaler, FixedLossScaler):
        raise NotImplementedError(f"TRAIN.BACKEND: hip with TRAIN.LOSS.SCALER {type(scaler).__name__}: "
                                  "FixedLossScaler only")
    kind = "value" if scaler.fixed_weight <= 1e-9 else "gradient"
    return make(beta, loss_fn, scaler, nx, **form), kind


def make_optimizer(params, opt_cfg):
    """PicardBaseSolution.configure_optimizers (solution.py:94-126): torch.optim.<cls>(**kwargs) and
    an optional per-step torch.optim.lr_scheduler.<cls> (ReduceLROnPlateau: patience 512 unless
    given, stepped on the training loss)."""
    opt = getattr(torch.optim, opt_cfg["cls"])(params, **dict(opt_cfg.get("kwargs") or {}))
    sched_cfg = opt_cfg.get("SCHEDULER") or {}
    sched = None
    if sched_cfg.get("cls") is not None:
        cls = getattr(torch.optim.lr_scheduler, sched_cfg["cls"])
        kws = {"patience": 512} if cls is torch.optim.lr_scheduler.ReduceLROnPlateau else {}
        kws.update(dict(sched_cfg.get("kwargs") or {}))
        sched = cls(opt, **kws)
    return opt, sched


def train_steps(net, objective, opt, batches, sched=None):
    """One optimizer step per (tx, y) batch, in the order Lightning's automatic optimisation runs
    them (training_step, zero_grad, backward, step, then the step-interval scheduler); returns the
    per-step losses as a device tensor (no host synchronisation per step)."""
    losses = []
    for tx, y in batches:
        loss, _ = objective(net, tx, y)
        opt.zero_grad()
        loss.sum().backward()
        opt.step()
        if sched is not None:
            if isinstance(sched, torch.optim.lr_scheduler.ReduceLROnPlateau):
                sched.step(loss.detach().sum())
            else:
                sched.step()
        losses.append(loss.detach().reshape(()))
    return torch.stack(losses) if losses else torch.empty(0)


def fused_train_steps(net, step, opt, batches, sched=None):
    """`train_steps` under TRAIN.FUSED_STEP: one `device_step` call per (tx, y) batch in place of objective,
    zero_grad, backward and opt.step, then the step-interval scheduler as there.  Returns the per-step
    total losses as a device tensor (no host synchronisation per step); the `info` of a step is
    `step_info` of the losses `step` returns.  No gradient tensor exists: `p.grad` stays None."""
    rows = []
    for tx, y in batches:
        losses = step(net, opt, tx, y)
        if sched is not None:
            if isinstance(sched, torch.optim.lr_scheduler.ReduceLROnPlateau):
                sched.step(losses[0])
            else:
                sched.step()
        rows.append(losses)
    return torch.stack(rows)[:, 0] if rows else torch.empty(0)
