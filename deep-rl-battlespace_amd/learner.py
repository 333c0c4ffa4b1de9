"""The learner's side of a PolicyRollout: the actor / value MLP as ONE fused forward and ONE fused backward (csrc/bsx_actor_grad.hip).

`StackedActor.forward` under torch autograd is ~20 memory-bound passes over [A, R, 64] activations forward and twice that backward, and it
saves every one of them.  `fused_apply` evaluates the same network with the rollout's own float32 kernel (`bsx_mlp_forward`:
bsx_actor_forward's kernel) and back-propagates with `bsx_mlp_grad` (bsx_actor_grad's kernel), which recomputes the forward in
registers: nothing is saved but the observations and the packed weights.  Deterministic (no floating-point atomics): the same inputs
give the same gradient bits on every call.  There is ONE path: fused_apply is fused_mlp on detached observation rows, fused_grad is
mlp_grad without the input gradient, and a network holds one set of cached buffers for all of them and for a PPOLearner.

  fused_apply(actor, obs, squash=True)                          the network, differentiable in the actor's ten parameters
  categorical_log_prob(actor, obs, actions, temperature, fused) the learner side of PolicyRollout(sample="categorical")
  rollout.gaussian_log_prob(..., fused=True)                    the learner side of sample="gaussian", through fused_apply
  fused_grad(actor, blob, obs, grad_out, squash)                the backward alone: mlp_grad(..., input_grad=False)[0], the [A, G] gradient row
  fused_mlp(net, x, squash=True)                                the same network on ANY input [..., A, D] (A <= 32, D <= 64: a Q critic on
                                                                obs (+) action), differentiable in the parameters and in x (bsx_mlp_grad)
  mlp_grad(net, blob, x, grad_out, squash, input_grad)          its backward alone, capturable: (the [A, G] gradient row, grad_x)
  split_grad(row, n_actions)                                    a [A, G] gradient row as the ten parameter shapes (views, no gather)
  ppo_head(kind, y, v, rec, logp_old, adv, ret, mask, ...)      the clipped-surrogate PPO loss between the two: from the forward's outputs
                                                                and a rollout's records to both grad_out tensors, one pass (bsx_ppo_head)
  AdamState(net_or_log_std), adam_step(nets, grads, states, ...) clip_grad_norm_ + Adam.step() + pack() of one or two networks (and log_std)
                                                                as two launches: rows in, parameters, moments and packed blobs out (bsx_adam_step)
  share_group(share, n), tie_(x, group), is_tied(x, group)      agents that share parameters: consecutive groups of `group` agents hold
                                                                identical networks; adam_step(..., group=g) steps a group with the sum of
                                                                its members' gradient rows (bsx_adam_step_shared)
  mlp_adam_step(nets, grads, states, blobs, hyper, step, ...)   the same step for any network fused_mlp takes (a Q critic, an odd A), with
                                                                Polyak target networks and their packed blobs kept in the same pass:
                                                                t = (1 - tau) t + tau p, tau = hyper[5] (bsx_adam_step_mlp)
  shuffle_rows(N, first, R, seed, seq, ...)                     a keyed permutation of [0, N) evaluated per position (bsx_shuffle_rows)
  minibatch_gather(src, dst, first, R, seed, seq, ...)          one shuffled minibatch's records through it, one launch (bsx_minibatch_gather)
  PPOLearner(rollout, ...)                                      minibatch_grads / update: the PPO update of a PolicyRollout's networks;
                                                                device_step=True: the whole update on device, capture() makes it one graph;
                                                                shuffle=True: a fresh permutation of the T x E rows per epoch;
                                                                share="team": one policy and one value function per team
  ddpg_inputs, ddpg_put_actions, td_head, ddpg_action_grad      what lies between the fused MLP calls of a DDPG update: the critic's
                                                                inputs from a sampled batch, a network's actions into them, the TD
                                                                target with both grad_out tensors, the actor's grad_out from the
                                                                critic's input gradient (bsx_ddpg_*, bsx_td_head)
  DDPGLearner(buffer, actor, critic=None, ...)                  the MADDPG update of a team from its DeviceReplayBuffer: a central or
                                                                own critic, Polyak targets, capture() makes it one graph
"""
from collections import namedtuple
from functools import partial

import torch

from . import _lib
from ._args import _F32, _FLAG, _need, _number, _workspace

H = 64
# The ten parameters of a StackedActor in the order of bsx_actor_grad's [A, G] row (csrc/bsx_actor_layout.h holds the kernels' side of it):
# name, rows as a function of D = obs_len, columns in the row, and whether the parameter keeps only the first n_actions of those columns.
# grad_floats, split_grad, AdamState's shape and adam_step's parameter checks follow from it.
_D, _ONE, _HID = (lambda D: D), (lambda D: 1), (lambda D: H)
_TABLE = (("w1", _D, H, False), ("b1", _ONE, H, False), ("g1", _ONE, H, False), ("h1", _ONE, H, False),
          ("w2", _HID, H, False), ("b2", _ONE, H, False), ("g2", _ONE, H, False), ("h2", _ONE, H, False),
          ("w3", _HID, 4, True), ("b3", _ONE, 4, True))
PARAMS = tuple(name for name, *_ in _TABLE)


def grad_floats(obs_len):
    """G of bsx_actor_grad: w1[D][64] | b1 | g1 | h1 | w2[64][64] | b2 | g2 | h2 | w3[64][4] | b3[4]."""
    return sum(rows(obs_len) * cols for _, rows, cols, _ in _TABLE)


def _mlp_blob_floats(obs_len):
    """Floats per agent of StackedActor.pack()'s blob at any input width of the fused MLP kernels: W1A over obs_len rounded up to even,
    then W2A, the six vectors, W3P, b3 and W2B's three bfloat16 terms (blob_floats asks the library, which answers for an actor's widths)."""
    return H * ((obs_len + 1) & ~1) + grad_floats(0) + H * H * 3 // 2


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

    def get(self, R, A, D, device, lib, go=False, gx=False):
        """go=False: for a caller that brings its own 4-column grad_out (PPOLearner: the head's outputs) -- none is allocated."""
        key = (int(R), int(A), int(D), str(device))
        if key not in self.by_key:
            nb = _lib.c_size_t()
            _lib.check(lib.bsx_mlp_grad_workspace_bytes(R, A, D, _lib.ctypes.byref(nb)), "bsx_mlp_grad_workspace_bytes")
            self.by_key[key] = dict(ws=torch.empty(((nb.value + 3) // 4,), dtype=torch.float32, device=device),
                                    grad=torch.empty((A, grad_floats(D)), dtype=torch.float32, device=device), go=None, gx=None)
        buf = self.by_key[key]
        if go and buf["go"] is None:
            buf["go"] = torch.zeros((R, A, 4), dtype=torch.float32, device=device)
        if gx and buf["gx"] is None:
            buf["gx"] = torch.empty((R, A, D), dtype=torch.float32, device=device)
        return buf


def _buffers(net):
    """The network's one buffer cache: fused_apply, fused_mlp, fused_grad, mlp_grad and PPOLearner all go through it."""
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
                                     _lib.ctypes.byref(nz) if nz is not None else None, 0, 0, None, 0,
                                     torch.cuda.current_stream(obs.device).cuda_stream), "bsx_actor_forward")


def _mlp_grad(lib, buf, blob, x, go4, squash, gx=None):
    """bsx_mlp_grad on the current stream, unchecked, on a grad_out that already has the kernel's 4-column layout (mlp_grad's padded copy,
    or bsx_ppo_head's g_pi / g_v) -> buf's row.  gx: the [R, A, D] tensor grad_x is written to; None is bsx_actor_grad's kernel."""
    R, A, D = x.shape
    _lib.check(lib.bsx_mlp_grad(blob.data_ptr(), x.data_ptr(), go4.data_ptr(), R, A, D, int(bool(squash)), buf["grad"].data_ptr(),
                                gx.data_ptr() if gx is not None else None, buf["ws"].data_ptr(),
                                torch.cuda.current_stream(x.device).cuda_stream), "bsx_mlp_grad")
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
    lib = _lib.load()
    buf = _buffers(net).get(R, A, D, dev, lib, go=True, gx=input_grad)
    buf["go"][..., :na].copy_(grad_out)                          # padded to 4 columns: the others hold 0 from the allocation on
    gx = buf["gx"] if input_grad else None
    return _mlp_grad(lib, buf, blob, x, buf["go"], squash, gx), gx


def fused_grad(actor, blob, obs, grad_out, squash=True):
    """mlp_grad without the input gradient, for an actor on its observations -> the [A, G] gradient row alone: one launch of
    bsx_actor_grad's kernel.  mlp_grad's checks, and its cached buffers: the row is overwritten by the next call with the same key."""
    return mlp_grad(actor, blob, obs, grad_out, squash, input_grad=False)[0]


class _FusedMlp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, net, x, squash, *params):
        A, D, na, R = net.n_actors, net.obs_len, net.n_actions, x.shape[0]
        blob = net.pack()                                        # a fresh blob: backward reads THIS one, not the parameters of later
        y = torch.empty((R, A, 4), dtype=torch.float32, device=x.device)
        raw = None if squash else torch.empty((R, A), dtype=torch.float32, device=x.device)
        _lib.check(_lib.load().bsx_mlp_forward(blob.data_ptr(), x.data_ptr(), y.data_ptr(), raw.data_ptr() if raw is not None else None,
                                               R, A, D, torch.cuda.current_stream(x.device).cuda_stream), "bsx_mlp_forward")
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
    if fused:
        s = fused_apply(actor, obs)
    else:
        s = actor(obs.reshape(-1, A, D)).reshape(*obs.shape[:-1], actor.n_actions)
    lp = torch.log_softmax(s / temperature, dim=-1)
    logp = lp.gather(-1, actions.unsqueeze(-1)).squeeze(-1)
    entropy = -(lp.exp() * lp).sum(-1)
    return logp, entropy


# ------------------------------------------------------------------------------------------------ the PPO update
PpoHead = namedtuple("PpoHead", "g_pi g_v g_log_std stats")
KINDS = {"categorical": 0, "gaussian": 1, 0: 0, 1: 1}
STATS = ("n", "loss", "policy_loss", "value_loss", "entropy", "approx_kl", "clip_fraction", "reserved")


# the ranges of the hyper-parameters, stated once: ppo_head, adam_hyper, PPOLearner and set_lr all check through _hyper
_SHARE = (lambda x: 0.0 < x < 1.0, "a number in (0, 1)")
_WEIGHT = (lambda x: x >= 0.0, "a number >= 0")
_POSITIVE = (lambda x: x > 0.0, "a number > 0")
_BETA = (lambda x: 0.0 <= x < 1.0, "a number in [0, 1)")
_UNIT = (lambda x: 0.0 <= x <= 1.0, "a number in [0, 1]")
_HYPER = {"clip": _SHARE, "c_v": _WEIGHT, "c_e": _WEIGHT, "temperature": _POSITIVE, "vclip": _POSITIVE, "lr": _WEIGHT, "betas[0]": _BETA,
          "betas[1]": _BETA, "eps": _WEIGHT, "max_grad_norm": _WEIGHT, "tau": _UNIT, "gamma": _UNIT}       # (max_grad_norm 0: adam_hyper's spelling of "no clipping")


def _hyper(name, x, rng=None):
    return _number(x, name, *(rng or _HYPER[name]))


def ppo_head_workspace_bytes(R, A):
    """Bytes of the workspace ppo_head needs for R rows of A agents."""
    lib, nb = _lib.load(), _lib.c_size_t()
    _lib.check(lib.bsx_ppo_head_workspace_bytes(int(R), int(A), _lib.ctypes.byref(nb)), "bsx_ppo_head_workspace_bytes")
    return nb.value


def ppo_head(kind, y, v, rec, logp_old, adv, ret, mask, *, clip, c_v, c_e, temperature=1.0, log_std=None, v_old=None, vclip=None, out=None,
             workspace=None):
    """The clipped-surrogate PPO loss and its gradient with respect to the two networks' outputs, in one pass (csrc/bsx_ppo_head.hip,
    `bsx_ppo_head`; the exact contract is written out in include/battlespace_hip.h) -> PpoHead(g_pi, g_v, g_log_std, stats).

    kind: "categorical" (0) or "gaussian" (1).  y f32 [R, A, 4]: the policy network's forward output (bsx_actor_forward's scores); v f32
    [R, A]: the value head's; rec f32 [R, A, 4]: the rollout's `scores` record (categorical: the played action is its first arg-max, taken
    in-kernel; gaussian: the unclipped draws); logp_old, adv, ret f32 [R, A] and mask (uint8 or bool [R, A]): the rollout's records, rows
    flattened ([T, E] -> R; leading axes are flattened here as long as the tensors are contiguous).  log_std f32 [A, 3] (gaussian); v_old
    f32 [R, A] with vclip > 0 clips the value loss around the recorded value.  Loss per masked row: -surr + c_v lv - c_e H, averaged over
    the N masked rows.
    g_pi, g_v f32 [R, A, 4]: what bsx_actor_grad takes as grad_out for the actor (squash=True) and the critic (squash=False); g_log_std f32
    [A, 3] (None for categorical); stats f64 [8] on the device, in the order of learner.STATS.  Deterministic; three launches on the
    current stream, no host synchronisation.  out: optional (g_pi, g_v, g_log_std, stats) to write into and workspace (at least
    ppo_head_workspace_bytes(R, A) bytes, 8-byte aligned) -- pass both and nothing is allocated (a captured graph)."""
    if kind not in KINDS:
        raise ValueError(f"kind must be 'categorical' or 'gaussian', got {kind!r}")
    k = KINDS[kind]
    if not isinstance(y, torch.Tensor) or y.dim() < 3 or y.shape[-1] != 4:
        raise ValueError("y must be a float32 [R, A, 4] tensor")
    dev, A = y.device, y.shape[-2]
    R = y.numel() // (4 * A) if A else 0
    if dev.type != "cuda":
        raise ValueError("ppo_head runs on the GPU: y is on " + str(dev))
    if R < 1 or A < 2 or A % 2 or A > 2 * _lib.MAX_N:
        raise ValueError(f"y has shape {tuple(y.shape)}: R >= 1 and an even A in 2 .. {2 * _lib.MAX_N} are needed")
    lead = tuple(y.shape[:-2])
    need = partial(_need, dev=dev, anchor="y")
    need(y, "y", (*lead, A, 4), _F32)
    need(v, "v", (*lead, A), _F32)
    need(rec, "rec", (*lead, A, 4), _F32)
    need(logp_old, "logp_old", (*lead, A), _F32)
    need(adv, "adv", (*lead, A), _F32)
    need(ret, "ret", (*lead, A), _F32)
    need(mask, "mask", (*lead, A), _FLAG)
    clip = _hyper("clip", clip)
    c_v = _hyper("c_v", c_v)
    c_e = _hyper("c_e", c_e)
    temperature = _hyper("temperature", temperature)
    if (v_old is None) != (vclip is None):
        raise ValueError("v_old and vclip go together: the value loss is clipped around v_old by vclip, or not at all")
    if v_old is not None:
        need(v_old, "v_old", (*lead, A), _F32)
        vclip = _hyper("vclip", vclip)
    if k == 1:
        if log_std is None:
            raise ValueError("kind 'gaussian' needs log_std, a float32 [A, 3] tensor")
        need(log_std, "log_std", (A, 3), _F32)
    elif log_std is not None:
        raise ValueError("log_std belongs to kind 'gaussian'")
    if out is None:
        g_pi, g_v = torch.empty((*lead, A, 4), dtype=torch.float32, device=dev), torch.empty((*lead, A, 4), dtype=torch.float32, device=dev)
        g_ls = torch.empty((A, 3), dtype=torch.float32, device=dev) if k == 1 else None
        stats = torch.empty(8, dtype=torch.float64, device=dev)
    else:
        g_pi, g_v, g_ls, stats = out
        need(g_pi, "out g_pi", (*lead, A, 4), _F32)
        need(g_v, "out g_v", (*lead, A, 4), _F32)
        if k == 1:
            need(g_ls, "out g_log_std", (A, 3), _F32)
        need(stats, "out stats", (8,), (torch.float64,))
    workspace = _workspace(workspace, ppo_head_workspace_bytes(R, A), dev)
    io = _lib.BsxPpoIo(y.data_ptr(), v.data_ptr(), rec.data_ptr(), logp_old.data_ptr(), adv.data_ptr(), ret.data_ptr(), mask.data_ptr(),
                       v_old.data_ptr() if v_old is not None else None, log_std.data_ptr() if k == 1 else None,
                       g_pi.data_ptr(), g_v.data_ptr(), g_ls.data_ptr() if k == 1 else None)
    _lib.check(_lib.load().bsx_ppo_head(_lib.ctypes.byref(io), R, A, k, temperature, clip, vclip if v_old is not None else 0.0, c_v, c_e,
                                        workspace.data_ptr(), stats.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), "bsx_ppo_head")
    return PpoHead(g_pi, g_v, g_ls if k == 1 else None, stats)


# ------------------------------------------------------------------------------------------------ the optimiser step
HYPER = ("lr", "beta1", "beta2", "eps", "max_grad_norm", "tau", "reserved", "reserved")
ADAM_STATS = ("step", "grad_norm", "clip_coef", "lr")


class AdamState:
    """The Adam moments adam_step keeps for one network or for log_std: `m` and `v`, float32 zeros.  For a StackedActor they are [A, G]
    rows in bsx_actor_grad's layout (split_grad cuts them into the ten parameter shapes; the pad columns of w3 / b3 stay +0), for a
    tensor (the Gaussian head's log_std, [A, 3]) they have its shape."""

    def __init__(self, net_or_log_std):
        x = net_or_log_std
        if isinstance(x, torch.Tensor):
            shape, dev = tuple(x.shape), x.device
        else:
            shape, dev = (x.n_actors, grad_floats(x.obs_len)), x.w1.device
        self.m = torch.zeros(shape, dtype=torch.float32, device=dev)
        self.v = torch.zeros(shape, dtype=torch.float32, device=dev)


def adam_hyper(lr=3e-4, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=None, device="cuda", tau=0.0):
    """adam_step's `hyper`: float32 [8] on the device in the order of learner.HYPER; max_grad_norm None (or 0) = no clipping.  tau in
    [0, 1]: the Polyak rate of mlp_adam_step's targets (adam_step does not read it)."""
    lr = _hyper("lr", lr)
    try:
        b1, b2 = betas
    except (TypeError, ValueError):
        raise ValueError(f"betas must be a pair of numbers in [0, 1), got {betas!r}") from None
    b1 = _hyper("betas[0]", b1)
    b2 = _hyper("betas[1]", b2)
    eps = _hyper("eps", eps)
    mgn = 0.0 if max_grad_norm is None else _hyper("max_grad_norm", max_grad_norm)
    tau = _hyper("tau", tau)
    return torch.tensor([lr, b1, b2, eps, mgn, tau, 0.0, 0.0], dtype=torch.float32, device=device)


def share_group(share, n):
    """The agents per tied group of a 2n-agent network -> int.  share: None = 1 (every agent on its own), "team" = n (one set of
    parameters per team), "all" = 2n (one for everyone), or an int g: 1, or >= 2 and a divisor of n (consecutive blocks of g agents that
    never straddle the two teams), or 2n -- bsx_adam_step_shared's rule.  Agent a belongs to group a // g, whose leader is its first
    agent.  ValueError for anything else."""
    n = int(n)
    if n < 1:
        raise ValueError(f"n must be >= 1, got {n}")
    if share is None:
        return 1
    if isinstance(share, str):
        if share not in ("team", "all"):
            raise ValueError(f"share must be None, 'team', 'all' or an int, got {share!r}")
        return n if share == "team" else 2 * n
    if isinstance(share, bool) or not isinstance(share, int):
        raise ValueError(f"share must be None, 'team', 'all' or an int, got {share!r}")
    g = share
    if g != 1 and g != 2 * n and (g < 2 or n % g):
        raise ValueError(f"a group of {g} does not fit {n} agents a side: 1, a divisor of {n} that is >= 2, or {2 * n} are possible")
    return g


def _tied_tensors(x):
    """The [A, ...] tensors of x: a StackedActor's ten parameters, an AdamState's two moments, or x itself."""
    if isinstance(x, torch.Tensor):
        return [x]
    if isinstance(x, AdamState):
        return [x.m, x.v]
    if all(hasattr(x, k) for k in PARAMS):
        return [getattr(x, k) for k in PARAMS]
    raise TypeError("a StackedActor, an AdamState or an [A, ...] tensor is needed")


def _tied_group(t, group):
    """group checked against t's leading axis A = 2n -> (A, g)."""
    if t.dim() < 1 or t.shape[0] < 2 or t.shape[0] % 2:
        raise ValueError(f"a tensor of shape {tuple(t.shape)} has no leading axis of A = 2n agents")
    A = t.shape[0]
    if isinstance(group, bool) or not isinstance(group, int):
        raise ValueError(f"group must be an int (learner.share_group), got {group!r}")
    return A, share_group(group, A // 2)


def tie_(x, group):
    """Copy every group leader's slice over its group's members, in place and under no_grad -> x.  x: a StackedActor (all ten
    parameters), an AdamState (both moments) or an [A, ...] tensor such as log_std; group: share_group's int.  What PPOLearner(share=)
    asks of its networks, done BEFORE the rollout packs them (or followed by ro.fused.refresh() and critic.pack(out=ro._value_w))."""
    with torch.no_grad():
        for t in _tied_tensors(x):
            A, g = _tied_group(t, group)
            if g > 1:
                v = t.detach().view(A // g, g, *t.shape[1:])
                v.copy_(v[:, :1].clone().expand_as(v))
    return x


def is_tied(x, group):
    """Whether every member of every group of x (tie_'s argument) equals its leader -> bool; one host synchronisation."""
    ok = None
    for t in _tied_tensors(x):
        A, g = _tied_group(t, group)
        if g > 1:
            v = t.detach().view(A // g, g, *t.shape[1:])
            same = (v == v[:, :1]).all()
            ok = same if ok is None else ok & same
    return True if ok is None else bool(ok)


def adam_step_workspace_bytes(n, nets):
    """Bytes of the workspace adam_step needs for `nets` networks of 2n agents."""
    lib, nb = _lib.load(), _lib.c_size_t()
    _lib.check(lib.bsx_adam_step_workspace_bytes(int(n), int(nets), _lib.ctypes.byref(nb)), "bsx_adam_step_workspace_bytes")
    return nb.value


def adam_step(nets, grads, states, blobs, hyper, step, *, log_std=None, g_log_std=None, log_std_state=None, stats=None, workspace=None,
              group=1):
    """torch's clip_grad_norm_(params, max_grad_norm) + Adam.step() (no weight decay, no amsgrad) + StackedActor.pack(), as ONE device
    pass of two launches (csrc/bsx_adam_step.hip, `bsx_adam_step`; the exact contract is written out in include/battlespace_hip.h)
    -> stats f64 [4] on the device, in the order of learner.ADAM_STATS.

    nets: one or two StackedActors of the same A and D (float32, on one GPU, contiguous parameters): updated in place.  grads: per
    network the float32 [A, G] gradient row of bsx_actor_grad (fused_grad / PPOLearner.minibatch_grads), read only.  states: per
    network an AdamState.  blobs: per network a float32 [A, blob floats] tensor that receives, in every float, what net.pack() makes of
    the updated parameters (a rollout's `fused.weights`).  log_std, g_log_std (float32 [A, 3]) and log_std_state (an AdamState of it):
    the Gaussian head's, all three or none.  The global norm is taken over everything in the call.
    hyper: float32 [8] on the device (adam_hyper; learner.HYPER) and step: an int64 device tensor of one element, the steps taken so
    far, advanced by the call -- both are read on the device at every launch, so a captured call follows a changed learning rate and
    counts on from replay to replay.  The .grad of the parameters is neither read nor written.  Deterministic; no host synchronisation.
    stats (f64 [4]) and workspace (at least adam_step_workspace_bytes(n, len(nets)) bytes, 8-byte aligned): pass both and nothing is
    allocated (a captured graph).
    group > 1 (share_group) is the tied step, `bsx_adam_step_shared`: the agents in consecutive blocks of `group` share parameters.  The
    gradient of a group is the float32 sum of its members' rows in agent order (and of their g_log_std rows), it counts once in the
    global norm, and every member's parameters, moments and blob row are stepped with it from that member's own values -- members
    that are identical before the call (tie_) are identical after it.  group = 1 is the untied step, bit for bit."""
    return _adam_step("adam_step", False, nets, grads, states, blobs, hyper, step, log_std, g_log_std, log_std_state, stats, workspace, group)


def mlp_adam_step_workspace_bytes(A, nets):
    """Bytes of the workspace mlp_adam_step needs for `nets` networks of A agents (adam_step_workspace_bytes(n, nets) at A = 2n)."""
    lib, nb = _lib.load(), _lib.c_size_t()
    _lib.check(lib.bsx_adam_step_mlp_workspace_bytes(int(A), int(nets), _lib.ctypes.byref(nb)), "bsx_adam_step_mlp_workspace_bytes")
    return nb.value


def mlp_adam_step(nets, grads, states, blobs, hyper, step, *, targets=None, target_blobs=None, log_std=None, g_log_std=None,
                  log_std_state=None, stats=None, workspace=None, group=1):
    """adam_step for any StackedActor fused_mlp takes -- 1 .. 32 agents, odd counts allowed, 1 .. 64 inputs: a Q critic on obs (+) action
    -- with, per network, a Polyak target kept in the same two launches (`bsx_adam_step_mlp`, include/battlespace_hip.h) -> stats f64 [4].

    nets, grads, states, blobs, hyper, step, log_std, g_log_std, log_std_state, stats, workspace: adam_step's, word for word, with the
    workspace of mlp_adam_step_workspace_bytes(A, len(nets)).  At an actor's shape and without targets the call leaves adam_step's bits.
    targets: a list with, per network, a StackedActor of the same (A, D, n_actions) or None; target_blobs: a list with, per network, a
    float32 tensor of the shape of blobs[i] ([A, blob floats]: net.pack()'s) or None, matching targets.  After a network's step, per element in float32,
        t = (1 - tau) t + tau p,        tau = hyper[5] (adam_hyper(tau=)), read on the device at every launch,
    and target_blobs[i] receives, in every float, what targets[i].pack() makes of the blended target: what the next target forward
    (bsx_mlp_forward) reads.  The .grad of the targets is neither read nor written.
    group: any divisor of A, 1 = every agent on its own; the tied step of adam_step(group=) for consecutive blocks of `group` agents.
    Each member's target is blended with that member's own new parameters: targets tied before the call (tie_) are tied after it."""
    return _adam_step("mlp_adam_step", True, nets, grads, states, blobs, hyper, step, log_std, g_log_std, log_std_state, stats, workspace,
                      group, targets, target_blobs)


def _adam_step(what, free, nets, grads, states, blobs, hyper, step, log_std, g_log_std, log_std_state, stats, workspace, group,
               targets=None, target_blobs=None):
    """The one body of adam_step (free=False: an actor's shape, A = 2n and D = 3n + 2, share_group's groups, no targets) and mlp_adam_step
    (free=True: any shape of the fused MLP kernels, any group that divides A, Polyak targets): the checks in the order they fire, the
    argument structs, the call."""
    for name, x in (("nets", nets), ("grads", grads), ("states", states), ("blobs", blobs)):
        if not isinstance(x, (list, tuple)):
            raise TypeError(f"{name} must be a list or tuple, one entry per network")
    if len(nets) not in (1, 2) or not len(nets) == len(grads) == len(states) == len(blobs):
        raise ValueError("nets, grads, states and blobs must have one entry each for one or two networks")
    first = nets[0]
    if not all(hasattr(first, k) for k in PARAMS) or not isinstance(first.w1, torch.Tensor):
        raise TypeError("nets[0] must be a StackedActor")
    dev, A, D = first.w1.device, first.n_actors, first.obs_len
    with_targets = free and (targets is not None or target_blobs is not None)
    if with_targets:
        _check_targets(nets, targets, target_blobs)
    if dev.type != "cuda":
        raise ValueError(what + " runs on the GPU: nets[0].w1 is on " + str(dev))
    if free:
        if not 1 <= A <= 2 * _lib.MAX_N or not 1 <= D <= _lib.MLP_MAX_D:
            raise ValueError(f"nets[0] has {A} agents and obs_len {D}: 1 .. {2 * _lib.MAX_N} agents and 1 .. {_lib.MLP_MAX_D} inputs are needed")
    elif A < 2 or A % 2 or A > 2 * _lib.MAX_N or D != 3 * (A // 2) + 2:
        raise ValueError(f"nets[0] has {A} agents and obs_len {D}: an even A in 2 .. {2 * _lib.MAX_N} and D = 3 A / 2 + 2 are needed")
    G = grad_floats(D)
    if isinstance(group, bool) or not isinstance(group, int):
        raise ValueError(f"group must be an int (learner.share_group), got {group!r}")
    if not free:
        group = share_group(group, A // 2)
    elif group < 1 or A % group:
        raise ValueError(f"a group of {group} does not divide {A} agents")
    need = partial(_need, dev=dev, anchor="y")                   # ("y": the wording these messages have always had)
    io = _lib.BsxAdamIo()
    io.nets = len(nets)
    tg = _lib.BsxAdamTargets()
    for i, (net, g, st, blob) in enumerate(zip(nets, grads, states, blobs)):
        if not all(hasattr(net, k) for k in PARAMS):
            raise TypeError(f"nets[{i}] must be a StackedActor")
        if net.n_actors != A or net.obs_len != D:
            raise ValueError(f"nets[{i}] must have the {A} agents and obs_len {D} of nets[0]")
        na = net.n_actions
        if na not in (1, 3, 4):
            raise ValueError(f"nets[{i}].n_actions must be 1, 3 or 4, got {na}")
        for q, (k, rows, cols, cut) in enumerate(_TABLE):
            need(getattr(net, k), f"nets[{i}].{k}", (A, rows(D), na if cut else cols), _F32)
            io.net[i].p[q] = getattr(net, k).data_ptr()
        if not isinstance(st, AdamState):
            raise TypeError(f"states[{i}] must be an AdamState")
        need(g, f"grads[{i}]", (A, G), _F32)
        need(st.m, f"states[{i}].m", (A, G), _F32)
        need(st.v, f"states[{i}].v", (A, G), _F32)
        need(blob, f"blobs[{i}]", (A, _mlp_blob_floats(D)), _F32)
        io.net[i].grad, io.net[i].m, io.net[i].v, io.net[i].blob, io.net[i].n_actions = g.data_ptr(), st.m.data_ptr(), st.v.data_ptr(), blob.data_ptr(), na
        if with_targets and targets[i] is not None:
            for q, (k, rows, cols, cut) in enumerate(_TABLE):
                need(getattr(targets[i], k), f"targets[{i}].{k}", (A, rows(D), na if cut else cols), _F32)
                tg.net[i].p[q] = getattr(targets[i], k).data_ptr()
            need(target_blobs[i], f"target_blobs[{i}]", (A, _mlp_blob_floats(D)), _F32)
            tg.net[i].blob = target_blobs[i].data_ptr()
    given = [x is not None for x in (log_std, g_log_std, log_std_state)]
    if any(given) and not all(given):
        raise ValueError("log_std, g_log_std and log_std_state go together: all three or none")
    if all(given):
        if not isinstance(log_std_state, AdamState):
            raise TypeError("log_std_state must be an AdamState")
        need(log_std, "log_std", (A, 3), _F32)
        need(g_log_std, "g_log_std", (A, 3), _F32)
        need(log_std_state.m, "log_std_state.m", (A, 3), _F32)
        need(log_std_state.v, "log_std_state.v", (A, 3), _F32)
        io.log_std, io.g_log_std, io.m_ls, io.v_ls = log_std.data_ptr(), g_log_std.data_ptr(), log_std_state.m.data_ptr(), log_std_state.v.data_ptr()
    need(hyper, "hyper", (8,), _F32)
    if not isinstance(step, torch.Tensor):
        raise TypeError("step must be a torch.Tensor")
    need(step, "step", tuple(step.shape) if step.numel() == 1 else (1,), (torch.int64,))
    if stats is None:
        stats = torch.empty(4, dtype=torch.float64, device=dev)
    need(stats, "stats", (4,), (torch.float64,))
    workspace = _workspace(workspace, mlp_adam_step_workspace_bytes(A, len(nets)), dev)
    io.hyper, io.step = hyper.data_ptr(), step.data_ptr()
    stream = torch.cuda.current_stream(dev).cuda_stream
    lib, ref = _lib.load(), _lib.ctypes.byref
    if free:
        _lib.check(lib.bsx_adam_step_mlp(ref(io), A, D, group, ref(tg) if with_targets else None, workspace.data_ptr(), stats.data_ptr(),
                                         stream), "bsx_adam_step_mlp")
    elif group > 1:
        _lib.check(lib.bsx_adam_step_shared(ref(io), A // 2, group, workspace.data_ptr(), stats.data_ptr(), stream), "bsx_adam_step_shared")
    else:
        _lib.check(lib.bsx_adam_step(ref(io), A // 2, workspace.data_ptr(), stats.data_ptr(), stream), "bsx_adam_step")
    return stats


def _check_targets(nets, targets, target_blobs):
    """What mlp_adam_step asks of targets / target_blobs before any device is looked at: two lists of one entry per network, None in
    both or in neither, a StackedActor of its network's (A, D, n_actions), a tensor of the blob's shape."""
    if targets is None or target_blobs is None:
        raise ValueError("targets and target_blobs go together: both or neither")
    for name, x in (("targets", targets), ("target_blobs", target_blobs)):
        if not isinstance(x, (list, tuple)):
            raise TypeError(f"{name} must be a list or tuple, one entry (or None) per network")
        if len(x) != len(nets):
            raise ValueError(f"{name} must have one entry (or None) per network: {len(nets)}, got {len(x)}")
    for i, (net, t, tb) in enumerate(zip(nets, targets, target_blobs)):
        if (t is None) != (tb is None):
            raise ValueError(f"targets[{i}] and target_blobs[{i}] go together: both or None")
        if t is None:
            continue
        if not all(hasattr(t, k) for k in PARAMS):
            raise TypeError(f"targets[{i}] must be a StackedActor or None")
        if t is net:
            raise ValueError(f"targets[{i}] is nets[{i}] itself: a target is a network of its own")
        want = tuple(getattr(net, k, None) for k in ("n_actors", "obs_len", "n_actions"))
        have = (t.n_actors, t.obs_len, t.n_actions)
        if have != want:
            raise ValueError(f"targets[{i}] must have the (agents, obs_len, n_actions) = {want} of nets[{i}], got {have}")
        if not isinstance(tb, torch.Tensor):
            raise TypeError(f"target_blobs[{i}] must be a torch.Tensor")
        if tuple(tb.shape) != (t.n_actors, _mlp_blob_floats(t.obs_len)):
            raise ValueError(f"target_blobs[{i}] must have shape {(t.n_actors, _mlp_blob_floats(t.obs_len))}, got {tuple(tb.shape)}")


# ------------------------------------------------------------------------------------------------ shuffled minibatches
GATHER_ROWS = 32                         # destination rows per workgroup of bsx_minibatch_gather (csrc/bsx_shuffle.hip: ROWS)
_I64 = (torch.int64,)
# One minibatch's records, source or destination: obs f32 [rows, A, D], rec f32 [rows, A, 4], logp, adv, ret f32 [rows, A], mask uint8 or
# bool [rows, A], value f32 [rows, A] or None, and on the destination idx int64 [rows]
Minibatch = namedtuple("Minibatch", "obs rec logp adv ret mask value idx", defaults=(None, None))


def _word(x, name):
    """int(x) in [0, 2^64): a Philox seed or sequence number."""
    if isinstance(x, bool) or not isinstance(x, int) or not 0 <= x < 1 << 64:
        raise ValueError(f"{name} must be an int in [0, 2^64), got {x!r}")
    return x


def _rows(N, first, R):
    """(N, first, R) as ints: 1 <= N < 2^31 and a non-empty range [first, first + R) inside [0, N)."""
    N, first, R = int(N), int(first), int(R)
    if not 1 <= N < 1 << 31:
        raise ValueError(f"N must be in [1, 2^31), got {N}")
    if R < 1 or first < 0 or first + R > N:
        raise ValueError(f"rows [{first}, {first} + {R}) are not a non-empty range inside [0, {N})")
    return N, first, R


def _seq_base(seq_base, dev):
    if seq_base is None:
        return None
    if not isinstance(seq_base, torch.Tensor):
        raise TypeError("seq_base must be a torch.Tensor")
    _need(seq_base, "seq_base", tuple(seq_base.shape) if seq_base.numel() == 1 else (1,), _I64, dev, "the call's tensors")
    return seq_base.data_ptr()


def shuffle_rows(N, first, R, seed, seq, seq_base=None, out=None, device="cuda"):
    """Positions [first, first + R) of the keyed permutation of [0, N) (csrc/bsx_shuffle.hip, `bsx_shuffle_rows`; the construction is
    written out in include/battlespace_hip.h) -> int64 [R] on the device: the source row of every position.  A bijection of [0, N) for
    every (seed, seq + seq_base): seed, seq ints in [0, 2^64); seq_base an int64 device tensor of one element, read on the device at
    every launch (a captured call draws afresh once the caller advances it), or None.  One launch on the current stream, no host
    synchronisation.  out: an int64 [R] tensor to write into (nothing is allocated then); its device is the call's."""
    N, first, R = _rows(N, first, R)
    seed, seq = _word(seed, "seed"), _word(seq, "seq")
    if out is None:
        out = torch.empty(R, dtype=torch.int64, device=device)
    elif not isinstance(out, torch.Tensor):
        raise TypeError("out must be a torch.Tensor")
    dev = out.device
    if dev.type != "cuda":
        raise ValueError("shuffle_rows runs on the GPU: out is on " + str(dev))
    _need(out, "out", (R,), _I64, dev, "out")
    _lib.check(_lib.load().bsx_shuffle_rows(N, first, R, seed, seq, _seq_base(seq_base, dev), out.data_ptr(),
                                            torch.cuda.current_stream(dev).cuda_stream), "bsx_shuffle_rows")
    return out


def minibatch_gather(src, dst, first, R, seed, seq, seq_base=None):
    """One minibatch of a shuffled epoch in one launch (csrc/bsx_shuffle.hip, `bsx_minibatch_gather`): for r in [0, R), dst.idx[r] =
    perm(first + r) and row r of every field of dst = row dst.idx[r] of src, bit for bit -> dst.

    src, dst: a learner.Minibatch (or any sequence in its order).  src holds the N rows the permutation is over -- obs f32 [N, A, D]
    (leading axes are flattened: a rollout's [T, E, A, D] records are N = T E rows), rec f32 [N, A, 4], logp, adv, ret f32 [N, A], mask
    uint8 or bool [N, A], value f32 [N, A] or None --, dst the same fields with R rows and idx int64 [R]; value on both sides or on
    neither.  seed, seq, seq_base: shuffle_rows'.  The M calls first = m R of one (seed, seq) hold every source row exactly once.
    Contiguous tensors on one GPU; dst must not overlap src.  No host synchronisation, nothing allocated."""
    src, dst = Minibatch(*src), Minibatch(*dst)
    obs = src.obs
    if not isinstance(obs, torch.Tensor) or obs.dim() < 3:
        raise ValueError("src.obs must be a float32 [N, A, D] tensor")
    dev, A, D = obs.device, obs.shape[-2], obs.shape[-1]
    if dev.type != "cuda":
        raise ValueError("minibatch_gather runs on the GPU: src.obs is on " + str(dev))
    if A < 2 or A % 2 or A > 2 * _lib.MAX_N or not 1 <= D <= 3 * _lib.MAX_N + 2:
        raise ValueError(f"src.obs has shape {tuple(obs.shape)}: an even A in 2 .. {2 * _lib.MAX_N} and D in 1 .. {3 * _lib.MAX_N + 2} are needed")
    lead = tuple(obs.shape[:-2])
    N, first, R = _rows(obs.numel() // (A * D), first, R)
    seed, seq = _word(seed, "seed"), _word(seq, "seq")
    if (src.value is None) != (dst.value is None):
        raise ValueError("value goes on both sides or on neither: src.value and dst.value")
    need = partial(_need, dev=dev, anchor="src.obs")
    io = _lib.BsxMinibatchIo()
    for side, t, rows, pre in (("src", src, lead, ""), ("dst", dst, (R,), "dst_")):
        for f, tail, dtypes in (("obs", (A, D), _F32), ("rec", (A, 4), _F32), ("logp", (A,), _F32), ("adv", (A,), _F32), ("ret", (A,), _F32),
                                ("mask", (A,), _FLAG), ("value", (A,), _F32)):
            x = getattr(t, f)
            if f == "value" and x is None:
                continue
            need(x, f"{side}.{f}", (*rows, *tail), dtypes)
            setattr(io, pre + f, x.data_ptr())
    need(dst.idx, "dst.idx", (R,), _I64)
    io.idx = dst.idx.data_ptr()
    _lib.check(_lib.load().bsx_minibatch_gather(_lib.ctypes.byref(io), N, first, R, A, D, seed, seq, _seq_base(seq_base, dev),
                                                torch.cuda.current_stream(dev).cuda_stream), "bsx_minibatch_gather")
    return dst


def blob_floats(obs_len):
    """Floats per agent of the packed blob bsx_actor_forward reads (StackedActor.pack()): bsx_actor_blob_floats."""
    nf = _lib.c_int()
    _lib.check(_lib.load().bsx_actor_blob_floats(int(obs_len), _lib.ctypes.byref(nf)), "bsx_actor_blob_floats")
    return nf.value


class PPOLearner:
    """The PPO update of a PolicyRollout's two networks, on device:

        ro = PolicyRollout(env, actor, T, sample="categorical", temperature=0.7, value_actor=critic, gae=dict(gamma=0.99, lam=0.95, normalize=True))
        learner = PPOLearner(ro, epochs=4, minibatches=4)
        ro.start(); ro.capture()
        while training:
            ro.run()
            stats = learner.update()        # f64 [epochs * minibatches, 8] on the device, columns in the order of learner.STATS

    A minibatch is a contiguous range of whole ticks [t0, t1) (T % minibatches == 0): views of the tick-major records, no gather; every
    minibatch holds all E games.  minibatch_grads is five calls on the current stream -- pack both networks, ONE bsx_actor_forward that
    returns scores and value, bsx_ppo_head, bsx_mlp_grad (bsx_actor_grad's kernel) for the actor and for the critic -- with cached buffers: no host
    synchronisation, and nothing is allocated from the second call of a size on (pack's own temporaries aside), so it can be captured.
    update() runs epochs x minibatches of it in tick order, installs the gradients on the parameters (split_grad), clips their global
    norm if asked, steps the optimiser (torch Adam over both networks and, for the Gaussian head, log_std -- ~5 k floats per agent: not
    the hot path) and re-packs the rollout's weights, so that the next run() plays the updated policy.

    A rollout with a scripted opponent (PolicyRollout(opponent=instinct.Team(...))) trains the learned team only: the rollout's mask is 0
    on every row of a scripted agent, so the head's statistics (n, loss, approx_kl, clip_fraction, ...) and max_grad_norm's global norm
    are the learned team's, every gradient float of a scripted agent's networks and log_std row is +0, and an update leaves its
    parameters as they are (an optimiser with weight decay aside).

    device_step=True: the optimiser step is adam_step (bsx_adam_step) -- clipping, Adam(lr, betas, eps) and both packs in two launches
    that take the gradient rows as they are.  update() then calls neither install, torch's clipping, a torch optimiser nor pack(): a
    minibatch is five calls (ten launches), nothing is allocated from the second update on, and the parameters' .grad stays unset (None) on this
    path.  The blobs the step writes are the rollout's own (ro.fused.weights, ro._value_w), which minibatch_grads reads as well, so the
    next run() plays the updated policy with no refresh.  The learning rate and the step count live on the device (`hyper`,
    `step_count`): set_lr(x) changes the rate without a host synchronisation, `step_stats` (f64 [epochs * minibatches, 4], columns in the
    order of learner.ADAM_STATS) records step, gradient norm, clip coefficient and lr of every step.  A caller who edits the parameters
    from outside calls sync() to re-pack both blobs.  capture() records the whole update -- epochs x minibatches steps -- as ONE graph
    on one stream; update() replays it from then on.

    shuffle=True: every epoch cuts a fresh permutation of the T x E rows into the minibatches, instead of the same tick ranges in the same
    order.  Optimiser step i (epoch j = i // minibatches, minibatch m = i % minibatches) starts with ONE minibatch_gather of rows
    [m R, (m + 1) R), R = T E / minibatches, of the permutation keyed by (shuffle_seed, j + shuffle_base) into cached buffers of the
    unshuffled minibatch's size (shuffled_grads); the forward, the head, both backward calls and the step run on those.  `minibatch_idx`
    (int64 [epochs * minibatches, R]) holds the source rows of every step; `shuffle_base` (an int64 device word) moves by `epochs` at the
    end of every update, on the stream and inside a captured update, so every update and every replay shuffles afresh with no host work.
    Both optimiser paths take it.  shuffle_seed: an int in [0, 2^64); None takes the rollout's seed (the permutation's stream has a salt of
    its own).  shuffle=False (the default) is the tick-range path, bit for bit.

    share="team" / "all" / an int (share_group): parameter sharing, as MAPPO trains -- one policy and one value function per team, for
    everyone, or per block of g adjacent agents of a team.  The StackedActors keep their A slices; the members of a group hold
    identical ones, so the rollout, the forward, the backward and the loss are what they are without sharing, and the gradient of a
    shared parameter is the sum of its members' rows (the loss is a mean over all masked rows of all agents).  Tie first, then build:

        tie_(actor, g); tie_(critic, g); tie_(log_std, g)       # g = share_group("team", n); before PolicyRollout packs them
        ro = PolicyRollout(env, actor, T, ..., value_actor=critic, log_std=log_std)
        learner = PPOLearner(ro, share="team", device_step=True)

    (or tie and re-pack: ro.fused.refresh(); critic.pack(out=ro._value_w)).  The constructor checks is_tied on the actor, the critic and
    log_std -- one host synchronisation -- and raises a ValueError otherwise: it never ties for the caller.  `group` holds the group
    size.  device_step=True: every step is adam_step(group=g) -- the members' sum on the device, once in the global norm, every
    member stepped from its own values, so the members stay identical bit for bit; capture(), set_lr, sync and shuffle=True are
    unchanged.  device_step=False: install puts a group's sum on its leader's .grad slice and +0 on its followers', clipping and the
    optimiser run as without sharing, and the leaders' slices are copied over their followers after every step.  With a scripted
    opponent share="all" is a ValueError (the scripted team's parameters are left alone); share="team" trains the learned team's one
    policy and keeps every bit of the scripted team's.  share=None (the default) is the unshared update, bit for bit.

    rollout: a PolicyRollout with sample="categorical" or "gaussian", a value_actor and gae= (ValueError otherwise).  vclip: clip the
    value loss around the rollout's recorded values.  optimizer: any torch optimiser over the parameters, instead of Adam(lr, betas, eps)
    (a ValueError with device_step=True)."""

    def __init__(self, rollout, *, clip=0.2, c_v=0.5, c_e=0.01, vclip=None, epochs=4, minibatches=4, lr=3e-4, max_grad_norm=None, optimizer=None,
                 device_step=False, betas=(0.9, 0.999), eps=1e-8, shuffle=False, shuffle_seed=None, share=None):
        ro = rollout
        if getattr(ro, "_sample", None) is None and getattr(ro, "_gauss", None) is None:
            raise ValueError("PPOLearner needs a PolicyRollout with sample='categorical' or 'gaussian' (it reads the recorded logp)")
        if getattr(ro, "_value_w", None) is None or getattr(ro, "_gae", None) is None:
            raise ValueError("PPOLearner needs a PolicyRollout with a value_actor and gae= (it reads value, adv, ret and mask)")
        epochs, minibatches = int(epochs), int(minibatches)
        if epochs < 1 or minibatches < 1 or ro.T % minibatches:
            raise ValueError(f"epochs >= 1 and a minibatches >= 1 that divides T = {ro.T} are needed (a minibatch is a range of whole ticks)")
        if not isinstance(shuffle, bool):
            raise ValueError(f"shuffle must be True or False, got {shuffle!r}")
        if shuffle_seed is not None and not shuffle:
            raise ValueError("shuffle_seed belongs to shuffle=True")
        self.shuffle = shuffle
        self.shuffle_seed = (int(ro.fused.seed) & ((1 << 64) - 1) if shuffle_seed is None else _word(shuffle_seed, "shuffle_seed")) if shuffle else None
        self.rollout, self.actor, self.critic = ro, ro.actor, ro.value_actor
        self.kind = "gaussian" if ro._gauss is not None else "categorical"
        self.temperature = ro._sample["temperature"] if self.kind == "categorical" else 1.0
        self.log_std = ro.log_std if self.kind == "gaussian" else None
        self.clip = _hyper("clip", clip)
        self.c_v = _hyper("c_v", c_v)
        self.c_e = _hyper("c_e", c_e)
        self.vclip = None if vclip is None else _hyper("vclip", vclip)
        self.epochs, self.minibatches = epochs, minibatches
        self.max_grad_norm = None if max_grad_norm is None else _hyper("max_grad_norm", max_grad_norm, _POSITIVE)   # (no clipping is None here)
        _check_mlp(self.actor, ro.obs[:1], True, "fused_apply", obs_shaped=True)     # the observation check, under fused_apply's name
        _check_mlp(self.critic, ro.obs[:1], True, "fused_apply", obs_shaped=True)
        A = self.actor.n_actors
        self.group = share_group(share, A // 2)
        if self.group > 1:
            if getattr(ro, "opponent", None) is not None and self.group == A:
                raise ValueError("a rollout with a scripted opponent cannot share one policy across both teams (share='all'): the scripted "
                                 "team's parameters are left alone; use share='team'")
            for name, x in (("actor", self.actor), ("value_actor", self.critic), ("log_std", self.log_std)):
                if x is not None and not is_tied(x, self.group):
                    raise ValueError(f"share={share!r} needs networks that are already shared: the rollout's {name} differs inside a group of "
                                     f"{self.group} agents.  Tie actor, value_actor and log_std with learner.tie_(x, {self.group}) before "
                                     "building the PolicyRollout, or tie them and re-pack with ro.fused.refresh() and "
                                     "critic.pack(out=ro._value_w)")
        self.params = [getattr(self.actor, k) for k in PARAMS] + [getattr(self.critic, k) for k in PARAMS]
        if self.log_std is not None:
            self.params.append(self.log_std)
        dev = ro.obs.device
        self.device_step, self._graph = bool(device_step), None
        if self.device_step:
            if optimizer is not None:
                raise ValueError("device_step=True steps with bsx_adam_step: an optimizer= cannot be used with it")
            self.optimizer = None
            self.hyper = adam_hyper(lr, betas, eps, self.max_grad_norm, dev)
            self.step_count = torch.zeros(1, dtype=torch.int64, device=dev)
            self.adam_a, self.adam_v = AdamState(self.actor), AdamState(self.critic)
            self.adam_ls = AdamState(self.log_std) if self.log_std is not None else None
            self.step_stats = torch.zeros((epochs * minibatches, 4), dtype=torch.float64, device=dev)
            self._adam_ws = _workspace(None, adam_step_workspace_bytes(self.actor.n_actors // 2, 2), dev)
            self._blob_a, self._blob_v = ro.fused.weights, ro._value_w       # the step packs into the blobs the rollout plays from
        else:
            self.optimizer = optimizer if optimizer is not None else torch.optim.Adam(self.params, lr=lr, betas=betas, eps=eps)
            self._blob_a, self._blob_v = torch.empty_like(ro.fused.weights), torch.empty_like(ro._value_w)
        self._by_rows = {}
        self.stats = torch.zeros((epochs * minibatches, 8), dtype=torch.float64, device=dev)
        if shuffle:
            T, E, A, D = ro.T, *ro.obs.shape[1:]
            R = T * E // minibatches
            f = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)   # noqa: E731
            self.shuffle_base = torch.zeros(1, dtype=torch.int64, device=dev)
            self.minibatch_idx = torch.zeros((epochs * minibatches, R), dtype=torch.int64, device=dev)
            self._gathered = Minibatch(f(R, A, D), f(R, A, 4), f(R, A), f(R, A), f(R, A), torch.empty((R, A), dtype=torch.uint8, device=dev),
                                       f(R, A) if self.vclip is not None else None)

    def _head_buffers(self, R):
        """The forward's outputs and the head's, per row count: allocated once."""
        if R not in self._by_rows:
            A, dev = self.actor.n_actors, self.rollout.obs.device
            f = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)   # noqa: E731
            self._by_rows[R] = dict(y=f(R, A, 4), v=f(R, A), g_pi=f(R, A, 4), g_v=f(R, A, 4),
                                    g_ls=f(A, 3) if self.kind == "gaussian" else None,
                                    stats=torch.empty(8, dtype=torch.float64, device=dev),
                                    ws=_workspace(None, ppo_head_workspace_bytes(R, A), dev))
        return self._by_rows[R]

    def minibatch_grads(self, t0, t1, pack=True, stats=None):
        """The loss of ticks [t0, t1) of the rollout's current records under the CURRENT parameters -> (actor row [A, G], critic row
        [A, G], g_log_std [A, 3] or None, stats f64 [8]): the rows in bsx_actor_grad's layout (split_grad cuts them), all four cached
        buffers that the next call with the same tick count overwrites.  pack=False: the learner's blobs already hold the current
        parameters (adam_step wrote them) -- three launches fewer and no temporaries.  stats: an f64 [8] tensor the head writes
        instead of the cached one."""
        ro = self.rollout
        t0, t1 = int(t0), int(t1)
        if not 0 <= t0 < t1 <= ro.T:
            raise ValueError(f"ticks [{t0}, {t1}) are not a range inside the rollout's T = {ro.T}")
        E, A = ro.obs.shape[1:3]
        R = (t1 - t0) * E
        flat = lambda x: x[t0:t1].view(R, A, *x.shape[3:])                           # noqa: E731
        return self._grads(Minibatch(flat(ro.obs), flat(ro.scores), flat(ro.logp), flat(ro.adv), flat(ro.ret), flat(ro._mask),
                                     flat(ro.value) if self.vclip is not None else None), pack, stats)

    def shuffled_grads(self, i, pack=True, stats=None):
        """minibatch_grads for optimiser step i of a shuffled update (shuffle=True): epoch j = i // minibatches, minibatch m = i %
        minibatches.  ONE bsx_minibatch_gather -- N = T E rows, first = m R, R = T E / minibatches, keyed by (shuffle_seed, j +
        shuffle_base) -- copies the step's rows of obs[:T], scores, logp, adv, ret, mask (and value, with vclip) into cached buffers
        and their source rows into minibatch_idx[i]; the forward, the head and the two backward calls then run on those."""
        return self._grads(self._gather(i), pack, stats)

    def _gather(self, i):
        """Step i's rows into the cached buffers and their source rows into minibatch_idx[i] -> the buffers, a Minibatch."""
        if not self.shuffle:
            raise ValueError("shuffled_grads needs PPOLearner(shuffle=True)")
        ro, i = self.rollout, int(i)
        if not 0 <= i < self.epochs * self.minibatches:
            raise ValueError(f"step {i} is not one of the {self.epochs * self.minibatches} steps of an update")
        T, R = ro.T, self.minibatch_idx.shape[1]
        src = Minibatch(ro.obs[:T], ro.scores, ro.logp, ro.adv, ro.ret, ro._mask, ro.value if self.vclip is not None else None)
        minibatch_gather(src, self._gathered._replace(idx=self.minibatch_idx[i]), (i % self.minibatches) * R, R, self.shuffle_seed,
                         i // self.minibatches, self.shuffle_base)
        return self._gathered

    def _grads(self, mb, pack, stats):
        """The five calls of a minibatch on its records `mb` (a Minibatch of R contiguous rows: views of a tick range, or gathered)."""
        lib, obs = _lib.load(), mb.obs
        (R, A, D), dev = obs.shape, obs.device
        b = self._head_buffers(R)
        if pack:
            self.actor.pack(out=self._blob_a)
            self.critic.pack(out=self._blob_v)
        _actor_forward(lib, self._blob_a, obs, b["y"], self._blob_v, b["v"])
        head = ppo_head(self.kind, b["y"], b["v"], mb.rec, mb.logp, mb.adv, mb.ret, mb.mask,
                        clip=self.clip, c_v=self.c_v, c_e=self.c_e, temperature=self.temperature, log_std=self.log_std,
                        v_old=mb.value, vclip=self.vclip,
                        out=(b["g_pi"], b["g_v"], b["g_ls"], b["stats"] if stats is None else stats), workspace=b["ws"])
        # the head's outputs ARE bsx_mlp_grad's grad_out (four columns, the unused ones +0): mlp_grad's call without its padded copy
        row_a = _mlp_grad(lib, _buffers(self.actor).get(R, A, D, dev, lib), self._blob_a, obs, head.g_pi, True)
        row_v = _mlp_grad(lib, _buffers(self.critic).get(R, A, D, dev, lib), self._blob_v, obs, head.g_v, False)
        return row_a, row_v, head.g_log_std, head.stats

    def install(self, row_a, row_v, g_log_std):
        """The gradient rows onto the parameters' .grad (copies: the rows are overwritten by the next minibatch).  With share=: every
        group's sum (float32, in agent order from the leader's row on) on its leader's slice and +0 on its followers'."""
        with torch.no_grad():
            for net, row in ((self.actor, row_a), (self.critic, row_v)):
                for k, g in zip(PARAMS, split_grad(self._group_sum(row), net.n_actions)):
                    p = getattr(net, k)
                    if p.grad is None:
                        p.grad = torch.empty_like(p)
                    p.grad.copy_(g)
            if self.log_std is not None:
                if self.log_std.grad is None:
                    self.log_std.grad = torch.empty_like(self.log_std)
                self.log_std.grad.copy_(self._group_sum(g_log_std))

    def _group_sum(self, row):
        """row [A, ...] -> the same shape with every group's float32 sum, members added in agent order, at its leader and +0 at its
        followers (a new tensor); share=None: row itself."""
        g = self.group
        if g == 1:
            return row
        v = row.view(row.shape[0] // g, g, *row.shape[1:])
        out = torch.zeros_like(v)
        acc = v[:, 0].clone()
        for k in range(1, g):
            acc += v[:, k]
        out[:, 0] = acc
        return out.view(row.shape)

    def _tie_params(self):
        """The leaders' parameter slices over their followers (the torch path, after the optimiser's step)."""
        if self.group > 1:
            for x in (self.actor, self.critic, self.log_std):
                if x is not None:
                    tie_(x, self.group)

    def _schedule(self):
        """(i, t0, t1) of the optimiser steps of one update: epochs x minibatches, the minibatches in tick order in every epoch."""
        span = self.rollout.T // self.minibatches
        for i in range(self.epochs * self.minibatches):
            m = i % self.minibatches
            yield i, m * span, (m + 1) * span

    def update(self):
        """epochs x minibatches optimiser steps over the rollout's current records, the minibatches in tick order in every epoch (shuffle=True:
        a fresh permutation of the rows per epoch); then the rollout's packed weights are refreshed.  -> stats f64 [epochs * minibatches, 8] on the device (a cached buffer; no host sync)."""
        ro = self.rollout
        if self.device_step:
            if self._graph is not None:
                self._graph.replay()
            else:
                self._device_update()
            return self.stats
        for i, t0, t1 in self._schedule():
            row_a, row_v, g_ls, stats = self.shuffled_grads(i) if self.shuffle else self.minibatch_grads(t0, t1)
            self.install(row_a, row_v, g_ls)
            if self.max_grad_norm is not None:
                torch.nn.utils.clip_grad_norm_(self.params, self.max_grad_norm)
            self.optimizer.step()
            self._tie_params()
            self.stats[i].copy_(stats)
        ro.fused.refresh()
        self.critic.pack(out=ro._value_w)
        if self.shuffle:
            self.shuffle_base.add_(self.epochs)
        return self.stats

    # -------------------------------------------------------------------------------------------- device_step=True
    def _need_device_step(self, what):
        if not self.device_step:
            raise ValueError(f"{what} needs PPOLearner(device_step=True)")

    def _device_update(self):
        """epochs x minibatches times: the five-launch minibatch on the blobs as they stand, the head's statistics straight into
        stats[i], then adam_step on the rows.  Cached buffers only; no host synchronisation."""
        ls = self.log_std
        for i, t0, t1 in self._schedule():
            if self.shuffle:
                row_a, row_v, g_ls, _ = self.shuffled_grads(i, pack=False, stats=self.stats[i])
            else:
                row_a, row_v, g_ls, _ = self.minibatch_grads(t0, t1, pack=False, stats=self.stats[i])
            adam_step([self.actor, self.critic], [row_a, row_v], [self.adam_a, self.adam_v], [self._blob_a, self._blob_v], self.hyper,
                      self.step_count, log_std=ls, g_log_std=g_ls if ls is not None else None, log_std_state=self.adam_ls,
                      stats=self.step_stats[i], workspace=self._adam_ws, group=self.group)
        if self.shuffle:
            self.shuffle_base.add_(self.epochs)                  # on the stream, inside a captured update: the next one draws afresh

    def _state(self):
        """Every tensor an update writes that outlives it."""
        out = list(self.params) + [self.adam_a.m, self.adam_a.v, self.adam_v.m, self.adam_v.v, self.step_count, self._blob_a, self._blob_v,
                                   self.stats, self.step_stats]
        if self.adam_ls is not None:
            out += [self.adam_ls.m, self.adam_ls.v]
        if self.shuffle:
            out += [self.shuffle_base, self.minibatch_idx]
        return out

    def set_lr(self, lr):
        """The learning rate of the steps from now on, written to `hyper` on the device (a fill on the current stream: no host
        synchronisation); a captured update reads it at every replay."""
        self._need_device_step("set_lr")
        self.hyper[0].fill_(_hyper("lr", lr))

    def sync(self):
        """Re-pack both blobs from the parameters, once: for a caller who has edited the parameters from outside (loaded a checkpoint)."""
        self._need_device_step("sync")
        self.actor.pack(out=self._blob_a)
        self.critic.pack(out=self._blob_v)

    def capture(self):
        """Record the whole update() -- epochs x minibatches minibatches and steps -- as one graph on one stream; update() replays it from
        then on.  One eager update runs first as the warm-up (buffers, kernel modules) and is undone: capture() leaves parameters,
        moments, step count, blobs and statistics bit for bit as they were."""
        self._need_device_step("capture")
        dev = self.rollout.obs.device
        with torch.no_grad():
            keep = [t.detach().clone() for t in self._state()]
            self._device_update()
            for t, k in zip(self._state(), keep):
                t.detach().copy_(k)
        torch.cuda.synchronize(dev)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            self._device_update()
        self._graph = graph
        return self


# ------------------------------------------------------------------------------------------------ the DDPG / MADDPG update
TdHead = namedtuple("TdHead", "g_q g_pi td stats")
TD_STATS = ("n", "critic_loss", "q", "target", "abs_td", "done", "weight", "reserved")
MAX_OBS = 3 * _lib.MAX_N + 2


def _critic_width(nA, Do, k, central):
    """Dc of a critic input after the checks every ddpg_* call shares (bsx_ddpg_*'s ranges) -> int."""
    if not 1 <= nA <= _lib.MAX_N or not 1 <= Do <= MAX_OBS or k not in (3, 4):
        raise ValueError(f"1 .. {_lib.MAX_N} agents, observations of 1 .. {MAX_OBS} floats and 3 or 4 action columns are needed, got {nA}, {Do} and {k}")
    Dc = nA * (Do + k) if central else Do + k
    if Dc > _lib.MLP_MAX_D:
        raise ValueError(f"a central critic of {nA} agents reads {nA} x ({Do} + {k}) = {Dc} inputs: the fused MLP kernels take at most "
                         f"{_lib.MLP_MAX_D} (the reference's form fits up to 3v3: 9, 24 and 45 inputs; 4v4 central is 72) -- use critic_input='own'")
    return Dc


def _batch_rows(x, name):
    if not isinstance(x, torch.Tensor) or x.dim() != 3:
        raise ValueError(f"{name} must be a float32 [B, nA, columns] tensor")
    if x.device.type != "cuda":
        raise ValueError(f"the ddpg calls run on the GPU: {name} is on {x.device}")
    if not 1 <= x.shape[0] < 1 << 31:
        raise ValueError(f"{name} has {x.shape[0]} rows: 1 <= B < 2^31 is needed")
    return x.shape[0], x.shape[1], x.device


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _mlp_forward(lib, blob, x, y4, raw=None):
    """bsx_mlp_forward on the current stream, unchecked: the network packed in `blob` on x [R, A, D] -> y4 [R, A, 4] (tanh) and, with
    raw [R, A], head column 0 before tanh."""
    R, A, D = x.shape
    _lib.check(lib.bsx_mlp_forward(blob.data_ptr(), x.data_ptr(), y4.data_ptr(), raw.data_ptr() if raw is not None else None, R, A, D,
                                   _stream(x.device)), "bsx_mlp_forward")


def ddpg_inputs(obs, obs_next, act, *, central=True, out=None):
    """Everything of the critic's three inputs that comes from the sampled batch alone, in one launch (csrc/bsx_ddpg_head.hip,
    `bsx_ddpg_inputs`; include/battlespace_hip.h) -> (x_cur, x_next, x_pi), each float32 [B, nA, Dc].

    obs, obs_next float32 [B, nA, Do], act float32 [B, nA, k] (k = 3 or 4): a DeviceReplayBuffer's batch.  central=False: row (b, i) is
    obs[b, i] (+) a[b, i], Dc = Do + k; central=True: the team's joint observation and action, obs[b, 0] .. obs[b, nA-1] (+) a[b, 0] ..
    a[b, nA-1], Dc = nA (Do + k) <= 64.  x_cur is written whole (the replayed actions); x_next gets obs_next's columns and x_pi obs's,
    and with central=True every action slot of x_pi the replayed actions; the action columns ddpg_put_actions fills later are left as
    they are.  out: the three tensors to write into (nothing is allocated then); without it they are new and zero elsewhere."""
    B, nA, dev = _batch_rows(obs, "obs")
    Do, k = obs.shape[2], act.shape[2] if isinstance(act, torch.Tensor) and act.dim() == 3 else 0
    Dc = _critic_width(nA, Do, k, central)
    need = partial(_need, dev=dev, anchor="obs")
    need(obs, "obs", (B, nA, Do), _F32)
    need(obs_next, "obs_next", (B, nA, Do), _F32)
    need(act, "act", (B, nA, k), _F32)
    if out is None:
        out = tuple(torch.zeros((B, nA, Dc), dtype=torch.float32, device=dev) for _ in range(3))
    x_cur, x_next, x_pi = out
    for x, name in zip(out, ("out x_cur", "out x_next", "out x_pi")):
        need(x, name, (B, nA, Dc), _F32)
    batch = _lib.BsxDdpgBatch(obs.data_ptr(), obs_next.data_ptr(), act.data_ptr())
    _lib.check(_lib.load().bsx_ddpg_inputs(_lib.ctypes.byref(batch), B, nA, Do, k, int(bool(central)), x_cur.data_ptr(), x_next.data_ptr(),
                                           x_pi.data_ptr(), _stream(dev)), "bsx_ddpg_inputs")
    return x_cur, x_next, x_pi


def ddpg_put_actions(y4, x, obs_len, n_actions, *, central=True, own_only=False):
    """The first n_actions columns of a network's output rows y4 float32 [B, nA, 4] (bsx_mlp_forward's) into the action columns of the
    critic input x float32 [B, nA, Dc], in one launch (`bsx_ddpg_put_actions`) -> x.  own_only=False: row (b, i) receives the actions
    of all agents of row b (the target actors' actions into x_next); own_only=True: agent i's alone, into slot i (pi_i(o_i) into x_pi,
    whose other slots keep the replayed actions).  With central=False the two are the same.  Nothing else of x is written."""
    B, nA, dev = _batch_rows(y4, "y4")
    Do, k = int(obs_len), int(n_actions)
    Dc = _critic_width(nA, Do, k, central)
    need = partial(_need, dev=dev, anchor="y4")
    need(y4, "y4", (B, nA, 4), _F32)
    need(x, "x", (B, nA, Dc), _F32)
    _lib.check(_lib.load().bsx_ddpg_put_actions(y4.data_ptr(), B, nA, Do, k, int(bool(central)), int(bool(own_only)), x.data_ptr(),
                                                _stream(dev)), "bsx_ddpg_put_actions")
    return x


def ddpg_action_grad(gx, obs_len, n_actions, *, central=True, out=None):
    """Agent i's own action columns of row (b, i) of the critic's input gradient gx float32 [B, nA, Dc] (mlp_grad's grad_x on x_pi)
    -> g_a4 float32 [B, nA, 4]: the actor's grad_out as bsx_mlp_grad takes it (squash=True), column 3 +0 with three actions.  One
    launch (`bsx_ddpg_action_grad`).  out: the tensor to write into."""
    B, nA, dev = _batch_rows(gx, "gx")
    Do, k = int(obs_len), int(n_actions)
    Dc = _critic_width(nA, Do, k, central)
    need = partial(_need, dev=dev, anchor="gx")
    need(gx, "gx", (B, nA, Dc), _F32)
    if out is None:
        out = torch.empty((B, nA, 4), dtype=torch.float32, device=dev)
    need(out, "out", (B, nA, 4), _F32)
    _lib.check(_lib.load().bsx_ddpg_action_grad(gx.data_ptr(), B, nA, Do, k, int(bool(central)), out.data_ptr(), _stream(dev)),
               "bsx_ddpg_action_grad")
    return out


def td_head_workspace_bytes(B, nA):
    """Bytes of the workspace td_head needs for B rows of nA agents."""
    lib, nb = _lib.load(), _lib.c_size_t()
    _lib.check(lib.bsx_td_head_workspace_bytes(int(B), int(nA), _lib.ctypes.byref(nb)), "bsx_td_head_workspace_bytes")
    return nb.value


def td_head(q, q_next, rew, done, gamma, *, weight=None, out=None, workspace=None):
    """The TD target and both grad_out tensors of a DDPG update from the critic's outputs, in one pass (csrc/bsx_ddpg_head.hip,
    `bsx_td_head`; the exact contract is written out in include/battlespace_hip.h) -> TdHead(g_q, g_pi, td, stats).

    q, q_next, rew float32 [B, nA]: the critic on x_cur, the target critic on x_next (raw heads) and the rewards; done uint8 or bool
    [B, nA]; weight float32 [B, nA] or None (1 everywhere; the hook of a prioritised sampler); gamma in [0, 1].  Per element
    y = fmaf(gamma, done ? 0 : q_next, rew), d = q - y;  g_q[..., 0] = (w d) float(2 / B): the critic's grad_out (squash=False) for the
    sum over agents of mean_b w (Q - y)^2;  g_pi[..., 0] = -(w float(1 / B)): the seed of the critic's input-gradient pass for the sum
    over agents of -mean_b w Q;  td = y.  Columns 1 .. 3 of both are +0.  stats f64 [8] on the device in the order of learner.TD_STATS:
    means over the B nA elements.  Deterministic; two launches on the current stream, no host synchronisation.  out: optional
    (g_q, g_pi, td or None, stats) to write into and workspace (at least td_head_workspace_bytes(B, nA) bytes, 8-byte aligned) -- pass
    both and nothing is allocated (a captured graph)."""
    if not isinstance(q, torch.Tensor) or q.dim() != 2:
        raise ValueError("q must be a float32 [B, nA] tensor")
    dev, (B, nA) = q.device, q.shape
    if dev.type != "cuda":
        raise ValueError("td_head runs on the GPU: q is on " + str(dev))
    if not 1 <= B < 1 << 31 or not 1 <= nA <= _lib.MAX_N:
        raise ValueError(f"q has shape {tuple(q.shape)}: 1 <= B < 2^31 and 1 .. {_lib.MAX_N} agents are needed")
    gamma = _hyper("gamma", gamma)
    need = partial(_need, dev=dev, anchor="q")
    need(q, "q", (B, nA), _F32)
    need(q_next, "q_next", (B, nA), _F32)
    need(rew, "rew", (B, nA), _F32)
    need(done, "done", (B, nA), _FLAG)
    if weight is not None:
        need(weight, "weight", (B, nA), _F32)
    if out is None:
        f = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)       # noqa: E731
        out = (f(B, nA, 4), f(B, nA, 4), f(B, nA), torch.empty(8, dtype=torch.float64, device=dev))
    g_q, g_pi, td, stats = out
    need(g_q, "out g_q", (B, nA, 4), _F32)
    need(g_pi, "out g_pi", (B, nA, 4), _F32)
    if td is not None:
        need(td, "out td", (B, nA), _F32)
    need(stats, "out stats", (8,), (torch.float64,))
    workspace = _workspace(workspace, td_head_workspace_bytes(B, nA), dev)
    io = _lib.BsxTdIo(q.data_ptr(), q_next.data_ptr(), rew.data_ptr(), done.data_ptr(), weight.data_ptr() if weight is not None else None,
                      g_q.data_ptr(), g_pi.data_ptr(), td.data_ptr() if td is not None else None)
    _lib.check(_lib.load().bsx_td_head(_lib.ctypes.byref(io), B, nA, gamma, workspace.data_ptr(), stats.data_ptr(), _stream(dev)), "bsx_td_head")
    return TdHead(g_q, g_pi, td, stats)


class DDPGLearner:
    """The MADDPG update of a team from its replay ring, on device: per-agent actors, one critic per agent on the team's joint
    observation and action (critic_input="central", the reference's form; Lowe et al. 2017) or on the agent's own
    (critic_input="own": independent DDPG), soft target networks, Adam.

        buf = DeviceReplayBuffer(1_000_000, 512, env.possible_red, env.obs_size, env.obs_size * n, 4, seed=0)
        learner = DDPGLearner(buf, actor)                 # actor: StackedActor(n, obs_size, 4); a critic StackedActor(n, Dc, 1) is made
        learner.capture()
        while training:
            ro.run(); buf.append_rollout(ro, range(n))
            stats = learner.update()                      # f64 [updates, 8] on the device, columns in the order of learner.TD_STATS
            learner.publish(ro, range(n))                 # the rollout plays the updated actors

    One update, on the current stream, with cached buffers and no host synchronisation:
       1. buffer.sample()                                          the batch, drawn on the device
       2. ddpg_inputs                                              x_cur, and the batch's part of x_next and x_pi
       3. target actor on obs_next, ddpg_put_actions(own_only=False)   a' into x_next
       4. target critic on x_next -> q_next;  5. critic on x_cur -> q
       6. td_head                                                  y = r + gamma (1 - done) q_next, g_q, g_pi, the statistics
       7. mlp_grad of the critic on x_cur with g_q, mlp_adam_step of the critic with its target
       8. actor on obs, ddpg_put_actions(own_only=True)            pi_i(o_i) into slot i of x_pi; the other slots keep the replayed actions
       9. mlp_grad of the STEPPED critic on x_pi with g_pi -> grad_x, ddpg_action_grad
      10. mlp_grad of the actor on obs with that, mlp_adam_step of the actor with its target
    Every forward reads a packed blob (bsx_mlp_forward) that the steps keep current; nothing is allocated from the second update on.

    buffer: a DeviceReplayBuffer; its n_agents, observation size and n_actions give nA, Do and k, its batch_size B.  actor: a
    StackedActor(nA, Do, k) on the buffer's device; critic: a StackedActor(nA, Dc, 1), Dc = nA (Do + k) central (at most 64: up to 3v3)
    or Do + k own; one is made if none is given.  The learner owns deep copies of both as targets (`target_actor`, `target_critic`),
    the four packed blobs, two AdamStates, two hyper rows (adam_hyper with tau: `hyper_actor`, `hyper_critic`), two step counters, and
    the statistics: `stats` f64 [updates, 8] (TD_STATS) and `step_stats_actor` / `step_stats_critic` f64 [updates, 4] (ADAM_STATS).
    update() runs `updates` updates and returns `stats`; capture() records them as ONE graph, the ring's draw included, that update()
    replays from then on; set_lr writes the device hyper rows; sync() re-packs all four blobs after an outside edit of the networks;
    publish copies the actors into a rollout.  Parameter sharing, a second critic (TD3) and prioritised sampling are not here
    (td_head's `weight` is the hook for the last)."""

    def __init__(self, buffer, actor, critic=None, *, critic_input="central", gamma=0.95, tau=0.01, lr_actor=1e-3, lr_critic=1e-3,
                 betas=(0.9, 0.999), eps=1e-8, max_grad_norm=None, updates=1):
        import copy
        from .replay import DeviceReplayBuffer
        from .rollout import StackedActor
        if not isinstance(buffer, DeviceReplayBuffer):
            raise ValueError("DDPGLearner needs a DeviceReplayBuffer (it samples on the device)")
        if critic_input not in ("central", "own"):
            raise ValueError(f"critic_input must be 'central' or 'own', got {critic_input!r}")
        self.buffer, self.central = buffer, critic_input == "central"
        nA, Do, k, B = buffer.n_agents, buffer.actor_states.shape[2], buffer.n_actions, buffer.batch_size
        dev = buffer.actor_states.device
        Dc = _critic_width(nA, Do, k, self.central)
        self.nA, self.Do, self.k, self.B, self.Dc = nA, Do, k, B, Dc
        self.gamma = _hyper("gamma", gamma)
        self.updates = int(updates)
        if self.updates < 1:
            raise ValueError(f"updates must be >= 1, got {updates!r}")
        mgn = None if max_grad_norm is None else _hyper("max_grad_norm", max_grad_norm, _POSITIVE)
        if critic is None:
            critic = StackedActor(nA, Dc, 1, device=dev)
        for net, name, want in ((actor, "actor", (nA, Do, k)), (critic, "critic", (nA, Dc, 1))):
            have = tuple(getattr(net, a, None) for a in ("n_actors", "obs_len", "n_actions"))
            if not all(hasattr(net, p) for p in PARAMS) or have != want:
                raise ValueError(f"{name} must be a StackedActor{want} for this buffer and critic_input={critic_input!r}, got "
                                 f"{'StackedActor' + str(have) if None not in have else type(net).__name__}")
        f = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)       # noqa: E731
        self._x_cur, self._x_next, self._x_pi = f(B, nA, Dc), f(B, nA, Dc), f(B, nA, Dc)
        _check_mlp(actor, buffer._b_obs, True, "DDPGLearner")
        _check_mlp(critic, self._x_cur, False, "DDPGLearner")
        self.actor, self.critic = actor, critic
        self.target_actor, self.target_critic = copy.deepcopy(actor), copy.deepcopy(critic)
        for t in (self.target_actor, self.target_critic):
            t.__dict__.pop("_bsx_mlp_buffers", None)             # (a deep copy takes the network's cached buffers along)
            t.requires_grad_(False)
        self._blob_a, self._blob_c = actor.pack(), critic.pack()
        self._blob_ta, self._blob_tc = self.target_actor.pack(), self.target_critic.pack()
        self.adam_actor, self.adam_critic = AdamState(actor), AdamState(critic)
        self.hyper_actor = adam_hyper(lr_actor, betas, eps, mgn, dev, tau)
        self.hyper_critic = adam_hyper(lr_critic, betas, eps, mgn, dev, tau)
        self.step_actor, self.step_critic = (torch.zeros(1, dtype=torch.int64, device=dev) for _ in range(2))
        self.stats = torch.zeros((self.updates, 8), dtype=torch.float64, device=dev)
        self.step_stats_actor, self.step_stats_critic = (torch.zeros((self.updates, 4), dtype=torch.float64, device=dev) for _ in range(2))
        self._y4, self._yq4, self._g_q, self._g_pi, self._g_a4 = (f(B, nA, 4) for _ in range(5))
        self._q, self._q_next, self.td = f(B, nA), f(B, nA), f(B, nA)
        self._head_ws = _workspace(None, td_head_workspace_bytes(B, nA), dev)
        self._adam_ws = _workspace(None, mlp_adam_step_workspace_bytes(nA, 1), dev)
        lib = _lib.load()
        self._buf_a = _buffers(actor).get(B, nA, Do, dev, lib)
        self._buf_c = _buffers(critic).get(B, nA, Dc, dev, lib, gx=True)
        self._graph = None

    def _update(self, u):
        """Update u of a call: the ten steps of the class's docstring."""
        lib, buf = _lib.load(), self.buffer
        buf.sample()
        obs, obs_next, act, rew, done = buf._b_obs, buf._b_obs_, buf._b_act, buf._b_rew, buf._b_done
        Do, k, c = self.Do, self.k, self.central
        ddpg_inputs(obs, obs_next, act, central=c, out=(self._x_cur, self._x_next, self._x_pi))
        _mlp_forward(lib, self._blob_ta, obs_next, self._y4)
        ddpg_put_actions(self._y4, self._x_next, Do, k, central=c, own_only=False)
        _mlp_forward(lib, self._blob_tc, self._x_next, self._yq4, self._q_next)
        _mlp_forward(lib, self._blob_c, self._x_cur, self._yq4, self._q)
        td_head(self._q, self._q_next, rew, done, self.gamma, out=(self._g_q, self._g_pi, self.td, self.stats[u]), workspace=self._head_ws)
        row_c = _mlp_grad(lib, self._buf_c, self._blob_c, self._x_cur, self._g_q, False)
        mlp_adam_step([self.critic], [row_c], [self.adam_critic], [self._blob_c], self.hyper_critic, self.step_critic,
                      targets=[self.target_critic], target_blobs=[self._blob_tc], stats=self.step_stats_critic[u], workspace=self._adam_ws)
        _mlp_forward(lib, self._blob_a, obs, self._y4)
        ddpg_put_actions(self._y4, self._x_pi, Do, k, central=c, own_only=True)
        _mlp_grad(lib, self._buf_c, self._blob_c, self._x_pi, self._g_pi, False, self._buf_c["gx"])
        ddpg_action_grad(self._buf_c["gx"], Do, k, central=c, out=self._g_a4)
        row_a = _mlp_grad(lib, self._buf_a, self._blob_a, obs, self._g_a4, True)
        mlp_adam_step([self.actor], [row_a], [self.adam_actor], [self._blob_a], self.hyper_actor, self.step_actor,
                      targets=[self.target_actor], target_blobs=[self._blob_ta], stats=self.step_stats_actor[u], workspace=self._adam_ws)

    def _run(self):
        for u in range(self.updates):
            self._update(u)

    def update(self):
        """`updates` updates, each on a fresh draw of the ring -> stats f64 [updates, 8] on the device (a cached buffer; no host
        synchronisation).  The ring must hold at least one row."""
        if self._graph is not None:
            self._graph.replay()
        else:
            self._run()
        return self.stats

    def _state(self):
        """Every tensor an update writes that outlives it."""
        out = [self.buffer._draws, self.step_actor, self.step_critic, self._blob_a, self._blob_c, self._blob_ta, self._blob_tc, self.stats,
               self.step_stats_actor, self.step_stats_critic]
        for st in (self.adam_actor, self.adam_critic):
            out += [st.m, st.v]
        for net in (self.actor, self.critic, self.target_actor, self.target_critic):
            out += [getattr(net, p) for p in PARAMS]
        return out

    def capture(self):
        """Record the whole update() -- `updates` updates, the ring's draws included -- as one graph on one stream; update() replays it
        from then on.  One eager update runs first as the warm-up and is undone: capture() leaves parameters, targets, moments, step
        counts, blobs, statistics and the ring's draw counter bit for bit as they were."""
        dev = self.buffer.actor_states.device
        with torch.no_grad():
            keep = [t.detach().clone() for t in self._state()]
            self._run()
            for t, kept in zip(self._state(), keep):
                t.detach().copy_(kept)
        torch.cuda.synchronize(dev)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            self._run()
        self._graph = graph
        return self

    def set_lr(self, actor=None, critic=None):
        """The learning rates of the steps from now on, written to the hyper rows on the device (fills on the current stream: no host
        synchronisation); a captured update reads them at every replay.  None leaves a rate as it is."""
        if actor is not None:
            self.hyper_actor[0].fill_(_hyper("lr", actor))
        if critic is not None:
            self.hyper_critic[0].fill_(_hyper("lr", critic))

    def sync(self):
        """Re-pack all four blobs from their networks, once: for a caller who has edited parameters or targets from outside."""
        for net, blob in ((self.actor, self._blob_a), (self.critic, self._blob_c), (self.target_actor, self._blob_ta),
                          (self.target_critic, self._blob_tc)):
            net.pack(out=blob)

    def publish(self, rollout, columns):
        """The team's actors into a PolicyRollout that plays them: the actor's blob rows into rollout.fused.weights[c0 : c0 + nA] (a blob
        row is per agent and depends on obs_len alone) and the ten parameter slices into rollout.actor.  columns: this team's env
        columns, a contiguous range, as append_rollout takes.  Device copies on the current stream (capturable); every other row of the
        rollout's blob and parameters is left untouched."""
        cols = [int(c) for c in columns]
        c0 = cols[0] if cols else 0
        ra = rollout.actor
        if len(cols) != self.nA or cols != list(range(c0, c0 + len(cols))) or c0 < 0 or c0 + len(cols) > ra.n_actors:
            raise ValueError(f"columns must be a contiguous range of {self.nA} of the rollout's {ra.n_actors} env columns")
        if (ra.obs_len, ra.n_actions) != (self.Do, self.k) or ra.w1.device != self.actor.w1.device:
            raise ValueError(f"the rollout's actor must have obs_len {self.Do} and {self.k} actions on {self.actor.w1.device}, got "
                             f"{ra.obs_len} and {ra.n_actions} on {ra.w1.device}")
        with torch.no_grad():
            if rollout.fused is not None:
                rollout.fused.weights[c0:c0 + self.nA].copy_(self._blob_a)
            for p in PARAMS:
                getattr(ra, p)[c0:c0 + self.nA].copy_(getattr(self.actor, p))
