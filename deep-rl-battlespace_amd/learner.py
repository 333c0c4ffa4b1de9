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
  ppo_head(kind, y, v, rec, logp_old, adv, ret, mask, ...)      the clipped-surrogate PPO loss between the two: from the forward's outputs
                                                                and a rollout's records to both grad_out tensors, one pass (bsx_ppo_head)
  PPOLearner(rollout, ...)                                      minibatch_grads / update: the PPO update of a PolicyRollout's networks
"""
import math
from collections import namedtuple

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

    def get(self, R, n, device, lib, go=True):
        """go=False: for a caller that brings its own 4-column grad_out (PPOLearner: the head's outputs) -- none is allocated."""
        key = (int(R), int(n), str(device))
        if key not in self.by_key:
            A, D = 2 * n, 3 * n + 2
            nb = _lib.c_size_t()
            _lib.check(lib.bsx_actor_grad_workspace_bytes(R, n, _lib.ctypes.byref(nb)), "bsx_actor_grad_workspace_bytes")
            self.by_key[key] = dict(ws=torch.empty(((nb.value + 3) // 4,), dtype=torch.float32, device=device),
                                    grad=torch.empty((A, grad_floats(D)), dtype=torch.float32, device=device), go=None)
        buf = self.by_key[key]
        if go and buf["go"] is None:
            buf["go"] = torch.zeros((R, 2 * n, 4), dtype=torch.float32, device=device)
        return buf


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
    return _actor_grad(lib, buf, blob, obs, go, squash)


def _actor_grad(lib, buf, blob, obs, go4, squash):
    """bsx_actor_grad on a grad_out that already has the kernel's 4-column layout (fused_grad's padded copy, or bsx_ppo_head's g_pi / g_v)."""
    R, A = obs.shape[0], obs.shape[1]
    _lib.check(lib.bsx_actor_grad(blob.data_ptr(), obs.data_ptr(), go4.data_ptr(), R, A // 2, int(bool(squash)), buf["grad"].data_ptr(),
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


# ------------------------------------------------------------------------------------------------ the PPO update
PpoHead = namedtuple("PpoHead", "g_pi g_v g_log_std stats")
KINDS = {"categorical": 0, "gaussian": 1, 0: 0, 1: 1}
STATS = ("n", "loss", "policy_loss", "value_loss", "entropy", "approx_kl", "clip_fraction", "reserved")
_F32, _FLAG = (torch.float32,), (torch.uint8, torch.bool)


def _need(x, name, shape, dtypes, dev):
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if x.dtype not in dtypes:
        raise TypeError(f"{name} must be {' or '.join(str(d) for d in dtypes)}, got {x.dtype}")
    if tuple(x.shape) != tuple(shape):
        raise ValueError(f"{name} must have shape {tuple(shape)}, got {tuple(x.shape)}")
    if x.device != dev:
        raise ValueError(f"{name} is on {x.device}, y on {dev}")
    if not x.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


def _number(x, name, ok, what):
    try:
        x = float(x)
        good = ok(x) and math.isfinite(x)
    except (TypeError, ValueError):
        good = False
    if not good:
        raise ValueError(f"{name} must be {what}, got {x!r}")
    return x


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
    _need(y, "y", (*lead, A, 4), _F32, dev)
    _need(v, "v", (*lead, A), _F32, dev)
    _need(rec, "rec", (*lead, A, 4), _F32, dev)
    _need(logp_old, "logp_old", (*lead, A), _F32, dev)
    _need(adv, "adv", (*lead, A), _F32, dev)
    _need(ret, "ret", (*lead, A), _F32, dev)
    _need(mask, "mask", (*lead, A), _FLAG, dev)
    clip = _number(clip, "clip", lambda x: 0.0 < x < 1.0, "a number in (0, 1)")
    c_v = _number(c_v, "c_v", lambda x: x >= 0.0, "a number >= 0")
    c_e = _number(c_e, "c_e", lambda x: x >= 0.0, "a number >= 0")
    temperature = _number(temperature, "temperature", lambda x: x > 0.0, "a number > 0")
    if (v_old is None) != (vclip is None):
        raise ValueError("v_old and vclip go together: the value loss is clipped around v_old by vclip, or not at all")
    if v_old is not None:
        _need(v_old, "v_old", (*lead, A), _F32, dev)
        vclip = _number(vclip, "vclip", lambda x: x > 0.0, "a number > 0")
    if k == 1:
        if log_std is None:
            raise ValueError("kind 'gaussian' needs log_std, a float32 [A, 3] tensor")
        _need(log_std, "log_std", (A, 3), _F32, dev)
    elif log_std is not None:
        raise ValueError("log_std belongs to kind 'gaussian'")
    if out is None:
        g_pi, g_v = torch.empty((*lead, A, 4), dtype=torch.float32, device=dev), torch.empty((*lead, A, 4), dtype=torch.float32, device=dev)
        g_ls = torch.empty((A, 3), dtype=torch.float32, device=dev) if k == 1 else None
        stats = torch.empty(8, dtype=torch.float64, device=dev)
    else:
        g_pi, g_v, g_ls, stats = out
        _need(g_pi, "out g_pi", (*lead, A, 4), _F32, dev)
        _need(g_v, "out g_v", (*lead, A, 4), _F32, dev)
        if k == 1:
            _need(g_ls, "out g_log_std", (A, 3), _F32, dev)
        _need(stats, "out stats", (8,), (torch.float64,), dev)
    nb = ppo_head_workspace_bytes(R, A)
    if workspace is None:
        workspace = torch.empty((nb + 7) // 8, dtype=torch.int64, device=dev)
    if (not isinstance(workspace, torch.Tensor) or workspace.device != dev or not workspace.is_contiguous()
            or workspace.numel() * workspace.element_size() < nb):
        raise ValueError(f"workspace must be a contiguous tensor of at least {nb} bytes on {dev}")
    io = _lib.BsxPpoIo(y.data_ptr(), v.data_ptr(), rec.data_ptr(), logp_old.data_ptr(), adv.data_ptr(), ret.data_ptr(), mask.data_ptr(),
                       v_old.data_ptr() if v_old is not None else None, log_std.data_ptr() if k == 1 else None,
                       g_pi.data_ptr(), g_v.data_ptr(), g_ls.data_ptr() if k == 1 else None)
    _lib.check(_lib.load().bsx_ppo_head(_lib.ctypes.byref(io), R, A, k, temperature, clip, vclip if v_old is not None else 0.0, c_v, c_e,
                                        workspace.data_ptr(), stats.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), "bsx_ppo_head")
    return PpoHead(g_pi, g_v, g_ls if k == 1 else None, stats)


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
    returns scores and value, bsx_ppo_head, bsx_actor_grad for the actor and for the critic -- with cached buffers: no host
    synchronisation, and nothing is allocated from the second call of a size on (pack's own temporaries aside), so it can be captured.
    update() runs epochs x minibatches of it in tick order, installs the gradients on the parameters (split_grad), clips their global
    norm if asked, steps the optimiser (torch Adam over both networks and, for the Gaussian head, log_std -- ~5 k floats per agent: not
    the hot path) and re-packs the rollout's weights, so that the next run() plays the updated policy.

    A rollout with a scripted opponent (PolicyRollout(opponent=instinct.Team(...))) trains the learned team only: the rollout's mask is 0
    on every row of a scripted agent, so the head's statistics (n, loss, approx_kl, clip_fraction, ...) and max_grad_norm's global norm
    are the learned team's, every gradient float of a scripted agent's networks and log_std row is +0, and an update leaves its
    parameters as they are (an optimiser with weight decay aside).

    rollout: a PolicyRollout with sample="categorical" or "gaussian", a value_actor and gae= (ValueError otherwise).  vclip: clip the
    value loss around the rollout's recorded values.  optimizer: any torch optimiser over the parameters, instead of Adam(lr)."""

    def __init__(self, rollout, *, clip=0.2, c_v=0.5, c_e=0.01, vclip=None, epochs=4, minibatches=4, lr=3e-4, max_grad_norm=None, optimizer=None):
        ro = rollout
        if getattr(ro, "_sample", None) is None and getattr(ro, "_gauss", None) is None:
            raise ValueError("PPOLearner needs a PolicyRollout with sample='categorical' or 'gaussian' (it reads the recorded logp)")
        if getattr(ro, "_value_w", None) is None or getattr(ro, "_gae", None) is None:
            raise ValueError("PPOLearner needs a PolicyRollout with a value_actor and gae= (it reads value, adv, ret and mask)")
        epochs, minibatches = int(epochs), int(minibatches)
        if epochs < 1 or minibatches < 1 or ro.T % minibatches:
            raise ValueError(f"epochs >= 1 and a minibatches >= 1 that divides T = {ro.T} are needed (a minibatch is a range of whole ticks)")
        self.rollout, self.actor, self.critic = ro, ro.actor, ro.value_actor
        self.kind = "gaussian" if ro._gauss is not None else "categorical"
        self.temperature = ro._sample["temperature"] if self.kind == "categorical" else 1.0
        self.log_std = ro.log_std if self.kind == "gaussian" else None
        self.clip = _number(clip, "clip", lambda x: 0.0 < x < 1.0, "a number in (0, 1)")
        self.c_v = _number(c_v, "c_v", lambda x: x >= 0.0, "a number >= 0")
        self.c_e = _number(c_e, "c_e", lambda x: x >= 0.0, "a number >= 0")
        self.vclip = None if vclip is None else _number(vclip, "vclip", lambda x: x > 0.0, "a number > 0")
        self.epochs, self.minibatches = epochs, minibatches
        self.max_grad_norm = None if max_grad_norm is None else _number(max_grad_norm, "max_grad_norm", lambda x: x > 0.0, "a number > 0")
        _check(self.actor, ro.obs[:1])
        _check(self.critic, ro.obs[:1])
        self.params = [getattr(self.actor, k) for k in PARAMS] + [getattr(self.critic, k) for k in PARAMS]
        if self.log_std is not None:
            self.params.append(self.log_std)
        self.optimizer = optimizer if optimizer is not None else torch.optim.Adam(self.params, lr=lr)
        dev = ro.obs.device
        self._blob_a, self._blob_v = torch.empty_like(ro.fused.weights), torch.empty_like(ro._value_w)
        self._by_rows = {}
        self.stats = torch.zeros((epochs * minibatches, 8), dtype=torch.float64, device=dev)

    def _head_buffers(self, R):
        """The forward's outputs and the head's, per row count: allocated once."""
        if R not in self._by_rows:
            A, dev = self.actor.n_actors, self.rollout.obs.device
            f = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)   # noqa: E731
            self._by_rows[R] = dict(y=f(R, A, 4), v=f(R, A), g_pi=f(R, A, 4), g_v=f(R, A, 4),
                                    g_ls=f(A, 3) if self.kind == "gaussian" else None,
                                    stats=torch.empty(8, dtype=torch.float64, device=dev),
                                    ws=torch.empty((ppo_head_workspace_bytes(R, A) + 7) // 8, dtype=torch.int64, device=dev))
        return self._by_rows[R]

    def minibatch_grads(self, t0, t1):
        """The loss of ticks [t0, t1) of the rollout's current records under the CURRENT parameters -> (actor row [A, G], critic row
        [A, G], g_log_std [A, 3] or None, stats f64 [8]): the rows in bsx_actor_grad's layout (split_grad cuts them), all four cached
        buffers that the next call with the same tick count overwrites."""
        ro, lib = self.rollout, _lib.load()
        t0, t1 = int(t0), int(t1)
        if not 0 <= t0 < t1 <= ro.T:
            raise ValueError(f"ticks [{t0}, {t1}) are not a range inside the rollout's T = {ro.T}")
        E, A, D = ro.obs.shape[1:]
        n, R, dev = A // 2, (t1 - t0) * E, ro.obs.device
        b = self._head_buffers(R)
        obs = ro.obs[t0:t1].view(R, A, D)
        self.actor.pack(out=self._blob_a)
        self.critic.pack(out=self._blob_v)
        nz = _lib.BsxActorNoise()
        nz.value_weights, nz.value = self._blob_v.data_ptr(), b["v"].data_ptr()
        _lib.check(lib.bsx_actor_forward(self._blob_a.data_ptr(), obs.data_ptr(), b["y"].data_ptr(), R, n, _lib.ACTOR_F32, _lib.ctypes.byref(nz),
                                         0, 0, None, 0, torch.cuda.current_stream(dev).cuda_stream), "bsx_actor_forward")
        flat = lambda x: x[t0:t1].view(R, A, *x.shape[3:])                           # noqa: E731
        head = ppo_head(self.kind, b["y"], b["v"], flat(ro.scores), flat(ro.logp), flat(ro.adv), flat(ro.ret), flat(ro._mask),
                        clip=self.clip, c_v=self.c_v, c_e=self.c_e, temperature=self.temperature, log_std=self.log_std,
                        v_old=flat(ro.value) if self.vclip is not None else None, vclip=self.vclip,
                        out=(b["g_pi"], b["g_v"], b["g_ls"], b["stats"]), workspace=b["ws"])
        # the head's outputs ARE bsx_actor_grad's grad_out (four columns, the unused ones +0): fused_grad's call without its padded copy
        row_a = _actor_grad(lib, _buffers(self.actor).get(R, n, dev, lib, go=False), self._blob_a, obs, head.g_pi, True)
        row_v = _actor_grad(lib, _buffers(self.critic).get(R, n, dev, lib, go=False), self._blob_v, obs, head.g_v, False)
        return row_a, row_v, head.g_log_std, head.stats

    def install(self, row_a, row_v, g_log_std):
        """The gradient rows onto the parameters' .grad (copies: the rows are overwritten by the next minibatch)."""
        with torch.no_grad():
            for net, row in ((self.actor, row_a), (self.critic, row_v)):
                for k, g in zip(PARAMS, split_grad(row, net.n_actions)):
                    p = getattr(net, k)
                    if p.grad is None:
                        p.grad = torch.empty_like(p)
                    p.grad.copy_(g)
            if self.log_std is not None:
                if self.log_std.grad is None:
                    self.log_std.grad = torch.empty_like(self.log_std)
                self.log_std.grad.copy_(g_log_std)

    def update(self):
        """epochs x minibatches optimiser steps over the rollout's current records, the minibatches in tick order in every epoch; then the
        rollout's packed weights are refreshed.  -> stats f64 [epochs * minibatches, 8] on the device (a cached buffer; no host sync)."""
        ro = self.rollout
        span, i = ro.T // self.minibatches, 0
        for _ in range(self.epochs):
            for m in range(self.minibatches):
                row_a, row_v, g_ls, stats = self.minibatch_grads(m * span, (m + 1) * span)
                self.install(row_a, row_v, g_ls)
                if self.max_grad_norm is not None:
                    torch.nn.utils.clip_grad_norm_(self.params, self.max_grad_norm)
                self.optimizer.step()
                self.stats[i].copy_(stats)
                i += 1
        ro.fused.refresh()
        self.critic.pack(out=ro._value_w)
        return self.stats
