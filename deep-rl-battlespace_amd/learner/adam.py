"""The optimiser step of the on-device learners (csrc/bsx_adam_step.hip): clip_grad_norm_ + Adam.step() + pack() as two launches.

  AdamState(net_or_log_std), adam_hyper(lr, betas, eps, ...)    the moments of one network (or of log_std) and the device row of rates
  adam_step(nets, grads, states, blobs, hyper, step, ...)       one or two actor-shaped networks (and log_std): rows in, parameters, moments, blobs out
  share_group(share, n), tie_(x, group), is_tied(x, group)      agents that share parameters; adam_step(group=g) steps a group with the sum of its rows
  mlp_adam_step(nets, grads, states, blobs, hyper, step, ...)   the same step for any network fused_mlp takes, with Polyak targets kept in the same pass
"""
from functools import partial

import torch

from .. import _lib
from .._args import _F32, _need, _workspace
from ._common import _hyper, _int64_word, _stream
from .mlp import PARAMS, _TABLE, _is_stacked, _mlp_blob_floats, grad_floats

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
        self.m, self.v = (torch.zeros(shape, dtype=torch.float32, device=dev) for _ in range(2))


def adam_hyper(lr=3e-4, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=None, device="cuda", tau=0.0):
    """adam_step's `hyper`: float32 [8] on the device in the order of learner.HYPER; max_grad_norm None (or 0) = no clipping.  tau in
    [0, 1]: the Polyak rate of mlp_adam_step's targets (adam_step does not read it)."""
    lr = _hyper("lr", lr)
    try:
        b1, b2 = betas
    except (TypeError, ValueError):
        raise ValueError(f"betas must be a pair of numbers in [0, 1), got {betas!r}") from None
    b1, b2, eps = _hyper("betas[0]", b1), _hyper("betas[1]", b2), _hyper("eps", eps)
    mgn = 0.0 if max_grad_norm is None else _hyper("max_grad_norm", max_grad_norm)
    return torch.tensor([lr, b1, b2, eps, mgn, _hyper("tau", tau), 0.0, 0.0], dtype=torch.float32, device=device)


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
    if isinstance(share, str) and share in ("team", "all"):
        return n if share == "team" else 2 * n
    if isinstance(share, (bool, str)) or not isinstance(share, int):
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
    if _is_stacked(x):
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
    return _lib.query_bytes("bsx_adam_step_workspace_bytes", n, nets)


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
    return _lib.query_bytes("bsx_adam_step_mlp_workspace_bytes", A, nets)


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
    if not _is_stacked(first) or not isinstance(first.w1, torch.Tensor):
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

    def ten(x, label, dst, na):
        """The ten parameters of x (nets[i] or targets[i], named `label`) at the network's n_actions: checked, their pointers into dst.p."""
        for q, (k, rows, cols, cut) in enumerate(_TABLE):
            need(getattr(x, k), f"{label}.{k}", (A, rows(D), na if cut else cols), _F32)
            dst.p[q] = getattr(x, k).data_ptr()

    io, tg = _lib.BsxAdamIo(), _lib.BsxAdamTargets()
    io.nets = len(nets)
    for i, (net, g, st, blob) in enumerate(zip(nets, grads, states, blobs)):
        if not _is_stacked(net):
            raise TypeError(f"nets[{i}] must be a StackedActor")
        if net.n_actors != A or net.obs_len != D:
            raise ValueError(f"nets[{i}] must have the {A} agents and obs_len {D} of nets[0]")
        na = net.n_actions
        if na not in (1, 3, 4):
            raise ValueError(f"nets[{i}].n_actions must be 1, 3 or 4, got {na}")
        ten(net, f"nets[{i}]", io.net[i], na)
        if not isinstance(st, AdamState):
            raise TypeError(f"states[{i}] must be an AdamState")
        for x, name in ((g, f"grads[{i}]"), (st.m, f"states[{i}].m"), (st.v, f"states[{i}].v")):
            need(x, name, (A, G), _F32)
        need(blob, f"blobs[{i}]", (A, _mlp_blob_floats(D)), _F32)
        io.net[i].grad, io.net[i].m, io.net[i].v, io.net[i].blob, io.net[i].n_actions = g.data_ptr(), st.m.data_ptr(), st.v.data_ptr(), blob.data_ptr(), na
        if with_targets and targets[i] is not None:
            ten(targets[i], f"targets[{i}]", tg.net[i], na)
            need(target_blobs[i], f"target_blobs[{i}]", (A, _mlp_blob_floats(D)), _F32)
            tg.net[i].blob = target_blobs[i].data_ptr()
    given = [x is not None for x in (log_std, g_log_std, log_std_state)]
    if any(given) and not all(given):
        raise ValueError("log_std, g_log_std and log_std_state go together: all three or none")
    if all(given):
        if not isinstance(log_std_state, AdamState):
            raise TypeError("log_std_state must be an AdamState")
        for x, name in ((log_std, "log_std"), (g_log_std, "g_log_std"), (log_std_state.m, "log_std_state.m"), (log_std_state.v, "log_std_state.v")):
            need(x, name, (A, 3), _F32)
        io.log_std, io.g_log_std, io.m_ls, io.v_ls = log_std.data_ptr(), g_log_std.data_ptr(), log_std_state.m.data_ptr(), log_std_state.v.data_ptr()
    need(hyper, "hyper", (8,), _F32)
    _int64_word(step, "step", dev, "y")
    if stats is None:
        stats = torch.empty(4, dtype=torch.float64, device=dev)
    need(stats, "stats", (4,), (torch.float64,))
    workspace = _workspace(workspace, mlp_adam_step_workspace_bytes(A, len(nets)), dev)
    io.hyper, io.step = hyper.data_ptr(), step.data_ptr()
    lib, ref, tail = _lib.load(), _lib.ctypes.byref, (workspace.data_ptr(), stats.data_ptr(), _stream(dev))
    if free:
        _lib.check(lib.bsx_adam_step_mlp(ref(io), A, D, group, ref(tg) if with_targets else None, *tail), "bsx_adam_step_mlp")
    elif group > 1:
        _lib.check(lib.bsx_adam_step_shared(ref(io), A // 2, group, *tail), "bsx_adam_step_shared")
    else:
        _lib.check(lib.bsx_adam_step(ref(io), A // 2, *tail), "bsx_adam_step")
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
        if not _is_stacked(t):
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
