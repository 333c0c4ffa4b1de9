"""The learner's side of a PolicyRollout: the actor / value MLP as ONE fused forward and ONE fused backward (csrc/bsx_actor_grad.hip).

`StackedActor.forward` under torch autograd is ~20 memory-bound passes over [A, R, 64] activations forward and twice that backward, and it
saves every one of them.  `fused_apply` evaluates the same network with the rollout's own float32 kernel (`bsx_actor_forward`) and
back-propagates with `bsx_actor_grad`, which recomputes the forward in registers: nothing is saved but the observations and the packed
weights.  Deterministic (no floating-point atomics): the same inputs give the same gradient bits on every call.

  fused_apply(actor, obs, squash=True)                          the network, differentiable in the actor's ten parameters
  categorical_log_prob(actor, obs, actions, temperature, fused) the learner side of PolicyRollout(sample="categorical")
  rollout.gaussian_log_prob(..., fused=True)                    the learner side of sample="gaussian", through fused_apply
  fused_grad(actor, blob, obs, grad_out, squash)                the backward alone: one bsx_actor_grad call, the [A, G] gradient row
  split_grad(row, n_actions)                                    a [A, G] gradient row as the ten parameter shapes (views, no gather)
"""
import torch

from . import _lib

PARAMS = ("w1", "b1", "g1", "h1", "w2", "b2", "g2", "h2", "w3", "b3")
H = 64


def grad_floats(obs_len):
    """G of bsx_actor_grad: w1[D][64] | b1 | g1 | h1 | w2[64][64] | b2 | g2 | h2 | w3[64][4] | b3[4]."""
    return H * obs_len + H * H + 6 * H + H * 4 + 4


def split_grad(row, n_actions):
    """row [A, G] (the layout of bsx_actor_grad's `grad`) -> the ten gradients in PARAMS order, shaped like a StackedActor's parameters:
    views of `row`; w3 / b3 cut to their first n_actions columns."""
    A, G = row.shape
    D = (G - (H * H + 6 * H + H * 4 + 4)) // H
    if grad_floats(D) != G:
        raise ValueError(f"a gradient row of {G} floats matches no observation length")
    out, o = [], 0

    def take(n):
        nonlocal o
        v = row[:, o:o + n]
        o += n
        return v
    out.append(take(H * D).view(A, D, H))
    out += [take(H).view(A, 1, H) for _ in range(3)]
    out.append(take(H * H).view(A, H, H))
    out += [take(H).view(A, 1, H) for _ in range(3)]
    out.append(take(H * 4).view(A, H, 4)[:, :, :n_actions])
    out.append(take(4).view(A, 1, 4)[:, :, :n_actions])
    return out


class _GradBuffers:
    """Per actor: the buffers of bsx_actor_grad by (R, n, device) -- the workspace, the kernel's [A, G] output row, the 4-column
    grad_out (columns beyond n_actions stay 0) -- so that a captured learner step does not allocate them again."""

    def __init__(self):
        self.by_key = {}

    def get(self, R, n, device, lib):
        key = (int(R), int(n), str(device))
        if key not in self.by_key:
            A, D = 2 * n, 3 * n + 2
            nb = _lib.c_size_t()
            _lib.check(lib.bsx_actor_grad_workspace_bytes(R, n, _lib.ctypes.byref(nb)), "bsx_actor_grad_workspace_bytes")
            self.by_key[key] = dict(ws=torch.empty(((nb.value + 3) // 4,), dtype=torch.float32, device=device),
                                    grad=torch.empty((A, grad_floats(D)), dtype=torch.float32, device=device),
                                    go=torch.zeros((R, A, 4), dtype=torch.float32, device=device))
        return self.by_key[key]


def _buffers(actor):
    b = actor.__dict__.get("_bsx_grad_buffers")
    if b is None:
        b = actor.__dict__["_bsx_grad_buffers"] = _GradBuffers()
    return b


def _check(actor, obs):
    ps = [getattr(actor, k) for k in PARAMS]
    if not isinstance(obs, torch.Tensor) or not obs.is_cuda or any(not p.is_cuda for p in ps):
        raise ValueError("fused_apply runs on the GPU: the actor and obs must be CUDA tensors")
    if obs.dtype != torch.float32 or any(p.dtype != torch.float32 for p in ps):
        raise ValueError("fused_apply is float32: the actor and obs must be float32")
    if actor.w1.shape[2] != H or actor.w2.shape[1] != H or actor.w2.shape[2] != H:
        raise ValueError("the fused actor kernels are built for fc1 = fc2 = 64")
    if obs.requires_grad:
        raise ValueError("fused_apply gives no gradient with respect to obs: pass a tensor that does not require grad")
    A, D = actor.n_actors, actor.obs_len
    if obs.dim() < 2 or tuple(obs.shape[-2:]) != (A, D) or A % 2 or D != 3 * (A // 2) + 2 or obs.numel() == 0:
        raise ValueError(f"obs must be [..., {A}, {D}] with A = 2n agents and D = 3n + 2")
    if obs.device != actor.w1.device:
        raise ValueError("the actor and obs must be on the same device")


class _FusedApply(torch.autograd.Function):
    @staticmethod
    def forward(ctx, actor, obs, squash, *params):
        lib = _lib.load()
        A, D, na = actor.n_actors, actor.obs_len, actor.n_actions
        n, R = A // 2, obs.shape[0]
        blob = actor.pack()                                      # a fresh blob: backward reads THIS one, not the parameters of later
        stream = torch.cuda.current_stream(obs.device).cuda_stream
        scores = torch.empty((R, A, 4), dtype=torch.float32, device=obs.device)
        if squash:
            _lib.check(lib.bsx_actor_forward(blob.data_ptr(), obs.data_ptr(), scores.data_ptr(), R, n, _lib.ACTOR_F32, None, 0, 0, None, 0,
                                             stream), "bsx_actor_forward")
            y = scores[..., :na]
        else:                                                    # the value path: the same blob once more as the value head
            value = torch.empty((R, A), dtype=torch.float32, device=obs.device)
            nz = _lib.BsxActorNoise()
            nz.value_weights, nz.value = blob.data_ptr(), value.data_ptr()
            _lib.check(lib.bsx_actor_forward(blob.data_ptr(), obs.data_ptr(), scores.data_ptr(), R, n, _lib.ACTOR_F32, _lib.ctypes.byref(nz),
                                             0, 0, None, 0, stream), "bsx_actor_forward")
            y = value.unsqueeze(-1)
        ctx.save_for_backward(obs, blob)
        ctx.actor, ctx.squash = actor, bool(squash)
        return y

    @staticmethod
    def backward(ctx, gy):
        obs, blob = ctx.saved_tensors
        row = fused_grad(ctx.actor, blob, obs, gy, ctx.squash)
        # the gradients handed to autograd are views of ONE copy of the row: a parameter's .grad may keep them, the cached row is
        # overwritten by the next call
        grads = split_grad(row.clone(), ctx.actor.n_actions)
        return (None, None, None, *[g if need else None for g, need in zip(grads, ctx.needs_input_grad[3:])])


def fused_grad(actor, blob, obs, grad_out, squash=True):
    """One bsx_actor_grad call on the current stream: the [A, G] gradient row (split_grad cuts it) of sum <grad_out, y> for the network
    packed in `blob` (actor.pack()) on obs float32 [R, A, D]; grad_out [R, A, n_actions].  The row, the workspace and the 4-column copy of
    grad_out are the actor's cached buffers for (R, n, device): the row is overwritten by the next call with the same key, and nothing is
    allocated from the second call on.  fused_apply's backward is this call."""
    lib = _lib.load()
    A, na = actor.n_actors, actor.n_actions
    n, R = A // 2, obs.shape[0]
    buf = _buffers(actor).get(R, n, obs.device, lib)
    go = buf["go"]
    go[..., :na].copy_(grad_out)                                 # padded to 4 columns: the others hold 0 from the allocation on
    _lib.check(lib.bsx_actor_grad(blob.data_ptr(), obs.data_ptr(), go.data_ptr(), R, n, int(bool(squash)), buf["grad"].data_ptr(),
                                  buf["ws"].data_ptr(), torch.cuda.current_stream(obs.device).cuda_stream), "bsx_actor_grad")
    return buf["grad"]


def fused_apply(actor, obs, squash=True):
    """actor(obs) as one HIP kernel forward and one backward: obs float32 [..., A, D] -> [..., A, n_actions], tanh-squashed (squash=True,
    an actor: exactly FusedActor's float32 scores) or the raw head (squash=False: a value head, n_actions = 1).  Differentiable in the
    ten parameters of `actor` (a StackedActor on the GPU, float32, fc1 = fc2 = 64) and NOT in obs.  The backward reads the blob the
    forward packed, so an optimiser step between the two does not move it; its workspace and output row are cached on the actor per
    (rows, n, device).  ValueError: tensors off the GPU, not float32, other hidden sizes, an obs that requires grad."""
    _check(actor, obs)
    if not squash and actor.n_actions != 1:
        raise ValueError("squash=False is the value head: a StackedActor with one output")
    A, D = actor.n_actors, actor.obs_len
    flat = obs.detach().reshape(-1, A, D).contiguous()
    y = _FusedApply.apply(actor, flat, bool(squash), *[getattr(actor, k) for k in PARAMS])
    return y.reshape(*obs.shape[:-1], actor.n_actions)


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
    if fused:
        s = fused_apply(actor, obs)
    else:
        s = actor(obs.reshape(-1, A, D)).reshape(*obs.shape[:-1], actor.n_actions)
    lp = torch.log_softmax(s / temperature, dim=-1)
    logp = lp.gather(-1, actions.unsqueeze(-1)).squeeze(-1)
    entropy = -(lp.exp() * lp).sum(-1)
    return logp, entropy
