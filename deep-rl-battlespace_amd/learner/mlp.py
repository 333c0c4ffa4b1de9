"""The actor / value MLP as ONE fused forward and ONE fused backward (csrc/bsx_actor_grad.hip).

`StackedActor.forward` under torch autograd is ~20 memory-bound passes over [A, R, 64] activations forward and twice that backward, and it
saves every one of them.  `fused_apply` evaluates the same network with the rollout's own float32 kernel (`bsx_mlp_forward`:
bsx_actor_forward's kernel) and back-propagates with `bsx_mlp_grad` (bsx_actor_grad's kernel), which recomputes the forward in
registers: nothing is saved but the observations and the packed weights.  Deterministic (no floating-point atomics): the same inputs
give the same gradient bits on every call.  There is ONE path: fused_apply is fused_mlp on detached observation rows, fused_grad is
mlp_grad without the input gradient, and a network holds one set of cached buffers for all of them and for the learners.

  fused_apply(actor, obs), fused_mlp(net, x)                    the network on observation rows / on ANY input [..., A, D] (a Q critic), differentiable
  mlp_grad(net, blob, x, grad_out, ...), fused_grad(...)        the backward alone, capturable: (the [A, G] gradient row, grad_x) / the row alone
  split_grad(row, n_actions), categorical_log_prob(...)         a row as the ten parameter shapes; the learner side of sample="categorical"
"""
from functools import partial

import torch

from .. import _lib
from .._args import _F32, _need
from ._common import _stream

H = 64
# The ten parameters of a StackedActor in the order of bsx_actor_grad's [A, G] row (csrc/bsx_actor_layout.h holds the kernels' side of it):
# name, rows as a function of D = obs_len, columns in the row, and whether the parameter keeps only the first n_actions of those columns.
# grad_floats, split_grad, AdamState's shape and adam_step's parameter checks follow from it.
_D, _ONE, _HID = (lambda D: D), (lambda D: 1), (lambda D: H)
_TABLE = (("w1", _D, H, False), ("b1", _ONE, H, False), ("g1", _ONE, H, False), ("h1", _ONE, H, False),
          ("w2", _HID, H, False), ("b2", _ONE, H, False), ("g2", _ONE, H, False), ("h2", _ONE, H, False),
          ("w3", _HID, 4, True), ("b3", _ONE, 4, True))
PARAMS = tuple(name for name, *_ in _TABLE)


def _is_stacked(x):
    """Whether x has a StackedActor's ten parameters (the duck type every binding takes; it sits here, next to PARAMS)."""
    return all(hasattr(x, k) for k in PARAMS)


def grad_floats(obs_len):
    """G of bsx_actor_grad: w1[D][64] | b1 | g1 | h1 | w2[64][64] | b2 | g2 | h2 | w3[64][4] | b3[4]."""
    return sum(rows(obs_len) * cols for _, rows, cols, _ in _TABLE)


def _mlp_blob_floats(obs_len):
    """Floats per agent of StackedActor.pack()'s blob at any input width of the fused MLP kernels: W1A over obs_len rounded up to even,
    then W2A, the six vectors, W3P, b3 and W2B's three bfloat16 terms (blob_floats asks the library, which answers for an actor's widths)."""
    return H * ((obs_len + 1) & ~1) + grad_floats(0) + H * H * 3 // 2


def blob_floats(obs_len):
    """Floats per agent of the packed blob bsx_actor_forward reads (StackedActor.pack()): bsx_actor_blob_floats."""
    nf = _lib.c_int()
    _lib.check(_lib.load().bsx_actor_blob_floats(int(obs_len), _lib.ctypes.byref(nf)), "bsx_actor_blob_floats")
    return nf.value


def split_grad(row, n_actions):
    """row [A, G] (the layout of bsx_actor_grad's `grad`) -> the ten gradients in PARAMS order, shaped like a StackedActor's parameters:
    views of `row`; w3 / b3 cut to their first n_actions columns."""
    A, G = row.shape
    D = (G - grad_floats(0)) // H
    if grad_floats(D) != G:
        raise ValueError(f"a gradient row of {G} floats matches no observation length")
    out, o = [], 0
    for _, rows, cols, cut in _TABLE:
        n = rows(D) * cols
        v = row[:, o:o + n].view(A, rows(D), cols)
        out.append(v[:, :, :n_actions] if cut else v)
        o += n
    return out


class _Buffers:
    """Per network: the buffers of bsx_mlp_grad by (R, A, D, device) -- the workspace and the kernel's [A, G] output row, and once asked for
    the 4-column grad_out (columns beyond n_actions stay 0) and grad_x -- so that a captured learner step does not allocate them again."""

    def __init__(self):
        self.by_key = {}

    def get(self, R, A, D, device, lib=None, go=False, gx=False):
        """go=False: for a caller that brings its own 4-column grad_out (PPOLearner: the head's outputs) -- none is allocated.  lib: unused."""
        key = (int(R), int(A), int(D), str(device))
        if key not in self.by_key:
            nb = _lib.query_bytes("bsx_mlp_grad_workspace_bytes", R, A, D)
            self.by_key[key] = dict(ws=torch.empty(((nb + 3) // 4,), dtype=torch.float32, device=device),
                                    grad=torch.empty((A, grad_floats(D)), dtype=torch.float32, device=device), go=None, gx=None)
        buf = self.by_key[key]
        if go and buf["go"] is None:
            buf["go"] = torch.zeros((R, A, 4), dtype=torch.float32, device=device)
        if gx and buf["gx"] is None:
            buf["gx"] = torch.empty((R, A, D), dtype=torch.float32, device=device)
        return buf


def _buffers(net):
    """The network's one buffer cache: fused_apply, fused_mlp, fused_grad, mlp_grad and both learners all go through it."""
    b = net.__dict__.get("_bsx_mlp_buffers")
    if b is None:
        b = net.__dict__["_bsx_mlp_buffers"] = _Buffers()
    return b


def _check_mlp(net, x, squash, what, obs_shaped=False):
    """The refusals of every fused path, in the order they fire.  obs_shaped: fused_apply's two on top, after the checks of the tensors
    and before those of the sizes -- an input that requires grad, and anything but observation rows (A = 2n agents, D = 3n + 2)."""
    ps = [getattr(net, k) for k in PARAMS]
    both = "the actor and obs" if obs_shaped else "the network and x"
    if not isinstance(x, torch.Tensor) or not x.is_cuda or any(not p.is_cuda for p in ps):
        raise ValueError(f"{what} runs on the GPU: {both} must be CUDA tensors")
    if x.dtype != torch.float32 or any(p.dtype != torch.float32 for p in ps):
        raise ValueError(f"{what} is float32: {both} must be float32")
    if net.w1.shape[2] != H or net.w2.shape[1] != H or net.w2.shape[2] != H:
        raise ValueError("the fused MLP kernels are built for fc1 = fc2 = 64")
    A, D = net.n_actors, net.obs_len
    if obs_shaped:
        if x.requires_grad:
            raise ValueError(f"{what} gives no gradient with respect to obs: pass a tensor that does not require grad")
        if x.dim() < 2 or tuple(x.shape[-2:]) != (A, D) or A % 2 or D != 3 * (A // 2) + 2 or x.numel() == 0:
            raise ValueError(f"obs must be [..., {A}, {D}] with A = 2n agents and D = 3n + 2")
    if not 1 <= A <= 2 * _lib.MAX_N or not 1 <= D <= _lib.MLP_MAX_D or net.n_actions not in (1, 3, 4):
        raise ValueError(f"the fused MLP kernels take 1 .. {2 * _lib.MAX_N} agents, 1 .. {_lib.MLP_MAX_D} inputs and 1, 3 or 4 outputs, "
                         f"got {A}, {D} and {net.n_actions}")
    if x.dim() < 2 or tuple(x.shape[-2:]) != (A, D) or x.numel() == 0:
        raise ValueError(f"x must be [..., {A}, {D}] and not empty, got {tuple(x.shape)}")
    if x.device != net.w1.device:
        raise ValueError(f"{both} must be on the same device")
    if not squash and net.n_actions != 1:
        raise ValueError("squash=False is the value head: a StackedActor with one output")


def _actor_forward(lib, blob, obs, scores, value_blob=None, value=None):
    """bsx_actor_forward on the current stream, float32 and without noise: the network packed in `blob` on obs [R, A, D] -> scores [R, A, 4];
    with value_blob and value [R, A], the value head packed in value_blob in the same launch."""
    R, A = obs.shape[0], obs.shape[1]
    nz = None
    if value_blob is not None:
        nz = _lib.BsxActorNoise()
        nz.value_weights, nz.value = value_blob.data_ptr(), value.data_ptr()
    _lib.check(lib.bsx_actor_forward(blob.data_ptr(), obs.data_ptr(), scores.data_ptr(), R, A // 2, _lib.ACTOR_F32,
                                     _lib.ctypes.byref(nz) if nz is not None else None, 0, 0, None, 0, _stream(obs.device)),
               "bsx_actor_forward")


def _mlp_forward(lib, blob, x, y4, raw=None):
    """bsx_mlp_forward on the current stream, unchecked: the network packed in `blob` on x [R, A, D] -> y4 [R, A, 4] (tanh) and, with
    raw [R, A], head column 0 before tanh."""
    R, A, D = x.shape
    _lib.check(lib.bsx_mlp_forward(blob.data_ptr(), x.data_ptr(), y4.data_ptr(), raw.data_ptr() if raw is not None else None, R, A, D,
                                   _stream(x.device)), "bsx_mlp_forward")


def _mlp_grad(lib, buf, blob, x, go4, squash, gx=None):
    """bsx_mlp_grad on the current stream, unchecked, on a grad_out that already has the kernel's 4-column layout (mlp_grad's padded copy,
    or bsx_ppo_head's g_pi / g_v) -> buf's row.  gx: the [R, A, D] tensor grad_x is written to; None is bsx_actor_grad's kernel."""
    R, A, D = x.shape
    _lib.check(lib.bsx_mlp_grad(blob.data_ptr(), x.data_ptr(), go4.data_ptr(), R, A, D, int(bool(squash)), buf["grad"].data_ptr(),
                                gx.data_ptr() if gx is not None else None, buf["ws"].data_ptr(), _stream(x.device)), "bsx_mlp_grad")
    return buf["grad"]


def mlp_grad(net, blob, x, grad_out, squash=True, input_grad=True):
    """One bsx_mlp_grad call on the current stream -> (row, grad_x): the [A, G] gradient row (split_grad cuts it) of sum <grad_out, y> for
    the network packed in `blob` (net.pack()) on x float32 [R, A, D], and the gradient of the same sum with respect to x, float32
    [R, A, D] (None with input_grad=False: the launch is then bsx_actor_grad's kernel).  grad_out: float32 [R, A, n_actions].  net: a
    StackedActor of any n_actors in 1 .. 32 and obs_len in 1 .. 64.  The capturable form: the row, grad_x, the workspace and the
    4-column copy of grad_out are the network's cached buffers for (R, A, D, device) -- ONE set per network, whichever of fused_apply,
    fused_mlp, fused_grad, mlp_grad or a PPOLearner asks: a row or grad_x one call returned is overwritten by the next call with the
    same key -- and nothing is allocated from the second call on.  The backward of fused_mlp and of fused_apply is this call.
    ValueError: fused_mlp's refusals, a blob or a grad_out of another shape."""
    _check_mlp(net, x, squash, "mlp_grad")
    A, D, na = net.n_actors, net.obs_len, net.n_actions
    if x.dim() != 3:
        raise ValueError(f"x must be [R, {A}, {D}], got {tuple(x.shape)}")
    R, dev = x.shape[0], x.device
    need = partial(_need, dev=dev, anchor="x")
    need(x, "x", (R, A, D), _F32)
    need(grad_out, "grad_out", (R, A, na), _F32)
    need(blob, "blob", (A, _mlp_blob_floats(D)), _F32)
    buf = _buffers(net).get(R, A, D, dev, go=True, gx=input_grad)
    buf["go"][..., :na].copy_(grad_out)                          # padded to 4 columns: the others hold 0 from the allocation on
    gx = buf["gx"] if input_grad else None
    return _mlp_grad(_lib.load(), buf, blob, x, buf["go"], squash, gx), gx


def fused_grad(actor, blob, obs, grad_out, squash=True):
    """mlp_grad without the input gradient, for an actor on its observations -> the [A, G] gradient row alone: one launch of
    bsx_actor_grad's kernel.  mlp_grad's checks, and its cached buffers: the row is overwritten by the next call with the same key."""
    return mlp_grad(actor, blob, obs, grad_out, squash, input_grad=False)[0]


class _FusedMlp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, net, x, squash, *params):
        A, na, R = net.n_actors, net.n_actions, x.shape[0]
        blob = net.pack()                                        # a fresh blob: backward reads THIS one, not the parameters of later
        y = torch.empty((R, A, 4), dtype=torch.float32, device=x.device)
        raw = None if squash else torch.empty((R, A), dtype=torch.float32, device=x.device)
        _mlp_forward(_lib.load(), blob, x, y, raw)
        ctx.save_for_backward(x, blob)
        ctx.net, ctx.squash = net, bool(squash)
        return y[..., :na] if squash else raw.unsqueeze(-1)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        x, blob = ctx.saved_tensors
        row, gx = mlp_grad(ctx.net, blob, x, gy.contiguous(), ctx.squash, input_grad=ctx.needs_input_grad[1])
        # copies: autograd may keep what it is handed (a parameter's .grad: views of ONE copy of the row), the cached buffers are
        # overwritten by the next call
        grads = split_grad(row.clone(), ctx.net.n_actions)
        return (None, gx.clone() if gx is not None else None, None, *[g if need else None for g, need in zip(grads, ctx.needs_input_grad[3:])])


def _apply(net, x, squash):
    """_FusedMlp on x [..., A, D] flattened to rows -> [..., A, n_actions]."""
    A, D = net.n_actors, net.obs_len
    y = _FusedMlp.apply(net, x.reshape(-1, A, D).contiguous(), bool(squash), *[getattr(net, k) for k in PARAMS])
    return y.reshape(*x.shape[:-1], net.n_actions)


def fused_apply(actor, obs, squash=True):
    """actor(obs) as one HIP kernel forward and one backward: obs float32 [..., A, D] -> [..., A, n_actions], tanh-squashed (squash=True,
    an actor: exactly FusedActor's float32 scores) or the raw head (squash=False: a value head, n_actions = 1).  Differentiable, once,
    in the ten parameters of `actor` (a StackedActor on the GPU, float32, fc1 = fc2 = 64) and NOT in obs: fused_mlp on observation rows
    (A = 2n, D = 3n + 2) that are detached -- the same forward and the same backward (mlp_grad without the input gradient, on the blob
    the forward packed: an optimiser step between the two does not move it), and the same cached buffers on the actor.
    ValueError: fused_mlp's refusals, an obs that requires grad, an obs that is not [..., 2n, 3n + 2]."""
    _check_mlp(actor, obs, squash, "fused_apply", obs_shaped=True)
    return _apply(actor, obs.detach(), squash)


def fused_mlp(net, x, squash=True):
    """net(x) as one HIP kernel forward and one backward, for an input that need not be an observation row: x float32 [..., A, D] ->
    [..., A, n_actions], tanh-squashed (squash=True) or the raw head (squash=False: a value or Q head, n_actions = 1).  net: a
    StackedActor on the GPU, float32, fc1 = fc2 = 64, with any n_actors in 1 .. 32, obs_len in 1 .. 64 and 1, 3 or 4 outputs -- a
    Q critic on obs (+) action, for one.  Differentiable in the ten parameters AND in x when x requires grad (the deterministic policy
    gradient: dQ/da back through the actor); once differentiable.  The backward is one mlp_grad call on the blob the forward packed;
    its buffers are cached on the network (mlp_grad says how).  At A = 2n, D = 3n + 2 the outputs and the parameter gradients are the
    bits of bsx_actor_forward and bsx_actor_grad.  ValueError: tensors off the GPU, not float32, other hidden sizes, sizes out of
    range, an x that is not [..., A, D], squash=False with more than one output."""
    _check_mlp(net, x, squash, "fused_mlp")
    return _apply(net, x, squash)


def categorical_log_prob(actor, obs, actions, temperature=1.0, fused=False):
    """The categorical policy head on the learner's side (what a PPO update takes the ratio of): (logp, entropy), each [..., E, A], of
    `actions` (int64 [..., E, A], indices 0..3) under softmax(tanh(actor(obs)) / temperature) -- the distribution
    PolicyRollout(sample="categorical") draws from.  The action a recorded tick played is the FIRST arg-max of its `scores[t]` row (the
    perturbed scores: what the step kernel's arg-max takes).  actor: a StackedActor with 4 outputs; obs: [..., E, A, D].  Differentiable
    in the actor's parameters; the float32 reference of what finish_row (csrc/bsx_actor_core.h) writes into `logp`.
    fused=True evaluates and back-propagates the network with fused_apply."""
    if not temperature > 0.0:
        raise ValueError("temperature must be > 0")
    A, D = obs.shape[-2], obs.shape[-1]
    s = fused_apply(actor, obs) if fused else actor(obs.reshape(-1, A, D)).reshape(*obs.shape[:-1], actor.n_actions)
    lp = torch.log_softmax(s / temperature, dim=-1)
    logp = lp.gather(-1, actions.unsqueeze(-1)).squeeze(-1)
    entropy = -(lp.exp() * lp).sum(-1)
    return logp, entropy
