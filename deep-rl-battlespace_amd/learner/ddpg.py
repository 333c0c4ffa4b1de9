"""The DDPG / MADDPG update on device (csrc/bsx_ddpg_head.hip): what lies between the fused MLP calls, and the learner around it.

  ddpg_inputs, ddpg_put_actions, td_head, ddpg_action_grad      the critic's inputs from a batch, actions into them, the TD target, the actor's grad_out
  DDPGLearner(buffer, actor, critic=None, ...)                  the MADDPG update of a team from its DeviceReplayBuffer; capture() makes it one graph
  _RingLearner                                                  what a learner on a device ring holds and does whatever its algorithm: a network's record,
                                                                the state list, update(), capture(), sync(), publish() -- DDPGLearner's, dqn.DQNLearner's and qmix.QMIXLearner's base
"""
import copy
from collections import namedtuple
from functools import partial

import torch

from .. import _lib
from .._args import _F32, _FLAG, _need, _workspace
from ..replay import DeviceReplayBuffer, PrioritizedReplayBuffer
from ..rollout import StackedActor
from ._common import _POSITIVE, _capture, _f32, _hyper, _ptr, _stream
from .adam import AdamState, adam_hyper, mlp_adam_step, mlp_adam_step_workspace_bytes
from .mlp import PARAMS, _buffers, _check_mlp, _is_stacked, _mlp_forward, _mlp_grad

TdHead = namedtuple("TdHead", "g_q g_pi td stats")
_Net = namedtuple("_Net", "net target blob target_blob adam buf q q_next g_q")      # a network as a learner holds it (DDPGLearner._net)
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


def _stacked_shape(net, name, want, context=""):
    """The refusal of a learner's network that is not a StackedActor of the shape `want` = (n_actors, obs_len, n_actions); context:
    what beside the buffer fixes that shape, as the message's clause (" and critic_input='central'")."""
    have = tuple(getattr(net, a, None) for a in ("n_actors", "obs_len", "n_actions"))
    if not _is_stacked(net) or have != want:
        raise ValueError(f"{name} must be a StackedActor{want} for this buffer{context}, got "
                         f"{'StackedActor' + str(have) if None not in have else type(net).__name__}")


def _batch_rows(x, name):
    if not isinstance(x, torch.Tensor) or x.dim() != 3:
        raise ValueError(f"{name} must be a float32 [B, nA, columns] tensor")
    if x.device.type != "cuda":
        raise ValueError(f"the ddpg calls run on the GPU: {name} is on {x.device}")
    if not 1 <= x.shape[0] < 1 << 31:
        raise ValueError(f"{name} has {x.shape[0]} rows: 1 <= B < 2^31 is needed")
    return x.shape[0], x.shape[1], x.device


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


def _head_rows(q, what, name="q1"):
    """The shape check of a call that takes [B, nA] rows: `q`, its first, gives B, nA and the device."""
    if not isinstance(q, torch.Tensor) or q.dim() != 2:
        raise ValueError(f"{name} must be a float32 [B, nA] tensor")
    dev, (B, nA) = q.device, q.shape
    if dev.type != "cuda":
        raise ValueError(f"{what} runs on the GPU: {name} is on {dev}")
    if not 1 <= B < 1 << 31 or not 1 <= nA <= _lib.MAX_N:
        raise ValueError(f"{name} has shape {tuple(q.shape)}: 1 <= B < 2^31 and 1 .. {_lib.MAX_N} agents are needed")
    return B, nA, dev


def _head_args(what, rows, done, gamma, weight, grads, out, workspace, per_agent=(), rows4=(), values=()):
    """The argument check td_head, td3_head, sac_head, dqn_head and qmix_head share -> (B, nA, dev, gamma, out, workspace).  rows: the (tensor, name)
    pairs of the float32 [B, nA] inputs, the first giving the shape; per_agent: those of the float32 [nA] ones; grads: the names of the
    [B, nA, 4] outputs.  rows4: the pairs of float32 [B, nA, 4] inputs (dqn_head's network rows; a None among them is left out) -- where
    there are any, the first of THEM gives the shape; values: the names of [B, nA] outputs that follow the grads (dqn_head's q).  out:
    (*grads, *values, td or None, stats) to write into, or None for new tensors; workspace: bsx_<what>_workspace_bytes(B, nA) bytes, or
    None for a new one."""
    first, anchor = (rows4 or rows)[0]
    if rows4:
        if not isinstance(first, torch.Tensor) or first.dim() != 3:
            raise ValueError(f"{anchor} must be a float32 [B, nA, 4] tensor")
        B, nA, dev = _head_rows(first[..., 0], what, anchor)
    else:
        B, nA, dev = _head_rows(first, what, anchor)
    gamma = _hyper("gamma", gamma)
    need = partial(_need, dev=dev, anchor=anchor)
    for x, name in rows4:
        if x is not None:
            need(x, name, (B, nA, 4), _F32)
    for x, name in rows:
        need(x, name, (B, nA), _F32)
    need(done, "done", (B, nA), _FLAG)
    for x, name in per_agent:
        need(x, name, (nA,), _F32)
    if weight is not None:
        need(weight, "weight", (B, nA), _F32)
    if out is None:
        f = _f32(torch.empty, dev)
        out = (*(f(B, nA, 4) for _ in grads), *(f(B, nA) for _ in values), f(B, nA), torch.empty(8, dtype=torch.float64, device=dev))
    *g, td, stats = out
    if len(g) != len(grads) + len(values):
        raise ValueError(f"out must be ({', '.join(tuple(grads) + tuple(values))}, td or None, stats)")
    for x, name in zip(g, grads):
        need(x, "out " + name, (B, nA, 4), _F32)
    for x, name in zip(g[len(grads):], values):
        need(x, "out " + name, (B, nA), _F32)
    if td is not None:
        need(td, "out td", (B, nA), _F32)
    need(stats, "out stats", (8,), (torch.float64,))
    return B, nA, dev, gamma, out, _workspace(workspace, _lib.query_bytes(f"bsx_{what}_workspace_bytes", B, nA), dev)


def td_head_workspace_bytes(B, nA):
    """Bytes of the workspace td_head needs for B rows of nA agents."""
    return _lib.query_bytes("bsx_td_head_workspace_bytes", B, nA)


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
    B, nA, dev, gamma, (g_q, g_pi, td, stats), workspace = _head_args("td_head", ((q, "q"), (q_next, "q_next"), (rew, "rew")), done, gamma, weight,
                                                                     ("g_q", "g_pi"), out, workspace)
    io = _lib.BsxTdIo(q.data_ptr(), q_next.data_ptr(), rew.data_ptr(), done.data_ptr(), _ptr(weight), g_q.data_ptr(), g_pi.data_ptr(), _ptr(td))
    _lib.check(_lib.load().bsx_td_head(_lib.ctypes.byref(io), B, nA, gamma, workspace.data_ptr(), stats.data_ptr(), _stream(dev)), "bsx_td_head")
    return TdHead(g_q, g_pi, td, stats)


class _RingLearner:
    """What the learners that update networks from a device ring share, and no learner on its own: DDPGLearner (with TD3Learner and
    SACLearner under it), dqn.DQNLearner and qmix.QMIXLearner.  A subclass calls `_ring` first and sets `B`, `nA`, `Do`, `k`, `stats`, `critics`
    (the list of its critics' records; empty without one), `_actor_net`, the record of the network a rollout plays, `_adam_ws` and
    `_steps`, the (step counter, step statistics) pairs of its optimiser steps; it writes `_update(u)`."""

    def _ring(self, buffer, gamma, updates, max_grad_norm):
        """The refusals every ring learner starts with -> max_grad_norm as adam_hyper takes it; sets `buffer`, `gamma`, `updates`,
        `_prioritized` and `_graph`."""
        if not isinstance(buffer, DeviceReplayBuffer):
            raise ValueError(f"{type(self).__name__} needs a DeviceReplayBuffer (it samples on the device)")
        self.buffer, self.gamma, self.updates = buffer, _hyper("gamma", gamma), int(updates)
        if self.updates < 1:
            raise ValueError(f"updates must be >= 1, got {updates!r}")
        self._prioritized, self._graph = isinstance(buffer, PrioritizedReplayBuffer), None
        return None if max_grad_norm is None else _hyper("max_grad_norm", max_grad_norm, _POSITIVE)

    def _net(self, net, D, critic=False, gx=False, members=None):
        """A network as the learner holds it -> _Net: with a deep copy as its target, both packed blobs, its AdamState and MLP buffers;
        a critic also with its q, q_next and g_q tensors, and it joins `critics`, the list the update's loops run over.  members: the
        network's member count where it is not the team's nA (qmix.QMIXLearner's mixer): its MLP buffers are that wide."""
        B, nA, dev = self.B, self.nA if members is None else int(members), self.buffer.actor_states.device
        target = copy.deepcopy(net)
        target.__dict__.pop("_bsx_mlp_buffers", None)            # (a deep copy takes the network's cached buffers along)
        target.requires_grad_(False)
        f = _f32(torch.zeros, dev)
        rec = _Net(net, target, net.pack(), target.pack(), AdamState(net), _buffers(net).get(B, nA, D, dev, gx=gx),
                   *((f(B, nA), f(B, nA), f(B, nA, 4)) if critic else (None, None, None)))
        if critic:
            self.critics.append(rec)
        return rec

    def _nets(self):
        """The records of every network the learner steps: the played network first, then the critics."""
        return [self._actor_net] + self.critics

    def _net_state(self):
        """Of every network: its blobs and moments, then its parameters and its target's."""
        return ([t for n in self._nets() for t in (n.blob, n.target_blob, n.adam.m, n.adam.v)]
                + [getattr(net, p) for n in self._nets() for net in (n.net, n.target) for p in PARAMS])

    def _adam_one(self, n, row, hyper, step, stats):
        """ONE mlp_adam_step of the network of record n, on its gradient row, with its Polyak target and both blobs."""
        mlp_adam_step([n.net], [row], [n.adam], [n.blob], hyper, step, targets=[n.target], target_blobs=[n.target_blob], stats=stats,
                      workspace=self._adam_ws)

    def _state(self):
        """Every tensor an update writes that outlives it."""
        return ([self.buffer._draws] + [s for s, _ in self._steps] + [self.stats] + [t for _, t in self._steps] + self._net_state()
                + ([self.buffer._leaves, self.buffer.tree, self.buffer.max_priority] if self._prioritized else []))

    def _run(self):
        for u in range(self.updates):
            self._update(u)

    def update(self):
        """`updates` updates, each on a fresh draw of the ring -> stats f64 [updates, 8] on the device (a cached buffer; no host
        synchronisation).  The ring must hold at least one row."""
        (self._graph.replay if self._graph is not None else self._run)()
        return self.stats

    def capture(self):
        """Record the whole update() -- `updates` updates, the ring's draws included -- as one graph on one stream; update() replays it
        from then on.  One eager update runs first as the warm-up and is undone: capture() leaves parameters, targets, moments, step
        counts, blobs, statistics, the ring's draw counter and (a prioritised ring) its priorities, tree and max_priority bit for bit as
        they were."""
        self._graph = _capture(self._run, self._state, self.buffer.actor_states.device)
        return self

    def sync(self):
        """Re-pack every blob from its network (two per network: four, six with a second critic, two for a DQNLearner, four for a QMIXLearner), once: for a caller who has edited
        parameters or targets from outside."""
        for n in self._nets():
            n.net.pack(out=n.blob)
            n.target.pack(out=n.target_blob)

    def publish(self, rollout, columns):
        """The team's actors into a PolicyRollout that plays them: the actor's blob rows into rollout.fused.weights[c0 : c0 + nA] (a blob
        row is per agent and depends on obs_len alone) and the ten parameter slices into rollout.actor.  columns: this team's env
        columns, a contiguous range, as append_rollout takes.  Device copies on the current stream (capturable); every other row of the
        rollout's blob and parameters is left untouched."""
        cols = [int(c) for c in columns]
        c0 = cols[0] if cols else 0
        ra, net = rollout.actor, self._actor_net.net
        if len(cols) != self.nA or cols != list(range(c0, c0 + len(cols))) or c0 < 0 or c0 + len(cols) > ra.n_actors:
            raise ValueError(f"columns must be a contiguous range of {self.nA} of the rollout's {ra.n_actors} env columns")
        if (ra.obs_len, ra.n_actions) != (self.Do, self.k) or ra.w1.device != net.w1.device:
            raise ValueError(f"the rollout's actor must have obs_len {self.Do} and {self.k} actions on {net.w1.device}, got "
                             f"{ra.obs_len} and {ra.n_actions} on {ra.w1.device}")
        with torch.no_grad():
            if rollout.fused is not None:
                rollout.fused.weights[c0:c0 + self.nA].copy_(self._actor_net.blob)
            for p in PARAMS:
                getattr(ra, p)[c0:c0 + self.nA].copy_(getattr(net, p))


class DDPGLearner(_RingLearner):
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
          (a PrioritizedReplayBuffer: with weight = buffer.weights, then buffer.update_priorities(q, y): the rows' new priorities)
       7. mlp_grad of the critic on x_cur with g_q, mlp_adam_step of the critic with its target
       8. actor on obs, ddpg_put_actions(own_only=True)            pi_i(o_i) into slot i of x_pi; the other slots keep the replayed actions
       9. mlp_grad of the STEPPED critic on x_pi with g_pi -> grad_x, ddpg_action_grad
      10. mlp_grad of the actor on obs with that, mlp_adam_step of the actor with its target
    Every forward reads a packed blob (bsx_mlp_forward) that the steps keep current; nothing is allocated from the second update on.
    Steps 3, 4 and 5, 6, 7 and 8 to 10 are methods (`_next_actions`, `_critics_forward`, `_head`, `_critics_step`, `_actor_half`) that run
    over `critics`, the list of the critics' records: learner.TD3Learner and SACLearner put a second critic on it and override singly.

    buffer: a DeviceReplayBuffer; its n_agents, observation size and n_actions give nA, Do and k, its batch_size B.  actor: a
    StackedActor(nA, Do, k) on the buffer's device; critic: a StackedActor(nA, Dc, 1), Dc = nA (Do + k) central (at most 64: up to 3v3)
    or Do + k own; one is made if none is given.  The learner owns deep copies of both as targets (`target_actor`, `target_critic`),
    the four packed blobs, two AdamStates, two hyper rows (adam_hyper with tau: `hyper_actor`, `hyper_critic`), two step counters, and
    the statistics: `stats` f64 [updates, 8] (TD_STATS) and `step_stats_actor` / `step_stats_critic` f64 [updates, 4] (ADAM_STATS).
    update() runs `updates` updates and returns `stats`; capture() records them as ONE graph, the ring's draw included, that update()
    replays from then on; set_lr writes the device hyper rows; sync() re-packs all four blobs after an outside edit of the networks;
    publish copies the actors into a rollout.  With a replay.PrioritizedReplayBuffer the draw of step 1 is proportional to the
    ring's priorities, step 6 weighs both losses by the batch's importance weights (`buffer.weights`; TD_STATS' `weight` column is their
    mean), and directly after it, before the critic's step, the rows drawn get new priorities from |q - y| (`buffer.update_priorities`):
    six more launches per update at 2^20 rows (the weights; five of the priority update), inside the same graph; with a plain DeviceReplayBuffer every launch is as it was.
    A second critic, smoothed targets and a delayed actor step (TD3) are learner.TD3Learner's, a stochastic policy with a learned spread
    and temperature (SAC) is learner.SACLearner's; parameter sharing is not here.  n-step targets need nothing here: fill the ring
    through replay.NStepAppender (rows with the folded n-step reward and obs_next up to n ticks on) and give the learner
    gamma=app.bootstrap_gamma, the appender's gamma^n; step 6 is then the n-step target."""

    def __init__(self, buffer, actor, critic=None, *, critic_input="central", gamma=0.95, tau=0.01, lr_actor=1e-3, lr_critic=1e-3,
                 betas=(0.9, 0.999), eps=1e-8, max_grad_norm=None, updates=1):
        mgn = self._ring(buffer, gamma, updates, max_grad_norm)
        if critic_input not in ("central", "own"):
            raise ValueError(f"critic_input must be 'central' or 'own', got {critic_input!r}")
        self.central = critic_input == "central"
        nA, Do, k, B = buffer.n_agents, buffer.actor_states.shape[2], buffer.n_actions, buffer.batch_size
        dev = buffer.actor_states.device
        Dc = _critic_width(nA, Do, k, self.central)
        self.nA, self.Do, self.k, self.B, self.Dc = nA, Do, k, B, Dc
        if critic is None:
            critic = StackedActor(nA, Dc, 1, device=dev)
        _stacked_shape(actor, "actor", (nA, Do, k), f" and critic_input={critic_input!r}")
        _stacked_shape(critic, "critic", (nA, Dc, 1), f" and critic_input={critic_input!r}")
        f = _f32(torch.zeros, dev)                               # zero-filled: what no kernel of an update writes stays +0
        self._x_cur, self._x_next, self._x_pi = f(B, nA, Dc), f(B, nA, Dc), f(B, nA, Dc)
        _check_mlp(actor, buffer._b_obs, True, type(self).__name__)
        _check_mlp(critic, self._x_cur, False, type(self).__name__)
        self.critics = []
        self._actor_net, c = self._net(actor, Do), self._net(critic, Dc, critic=True, gx=True)
        self.actor, self.target_actor, self._blob_a, self._blob_ta, self.adam_actor, self._buf_a = self._actor_net[:6]
        self.critic, self.target_critic, self._blob_c, self._blob_tc, self.adam_critic, self._buf_c = c[:6]
        self.hyper_actor, self.hyper_critic = (adam_hyper(lr, betas, eps, mgn, dev, tau) for lr in (lr_actor, lr_critic))
        self.step_actor, self.step_critic = (torch.zeros(1, dtype=torch.int64, device=dev) for _ in range(2))
        self.stats = torch.zeros((self.updates, 8), dtype=torch.float64, device=dev)
        self.step_stats_actor, self.step_stats_critic = (torch.zeros((self.updates, 4), dtype=torch.float64, device=dev) for _ in range(2))
        self._steps = [(self.step_actor, self.step_stats_actor), (self.step_critic, self.step_stats_critic)]
        self._y4, self._yq4, self._g_pi, self._g_a4 = (f(B, nA, 4) for _ in range(4))
        self.td = f(B, nA)
        self._head_ws = _workspace(None, td_head_workspace_bytes(B, nA), dev)        # (the three heads share one plan: one size)
        self._adam_ws = _workspace(None, mlp_adam_step_workspace_bytes(nA, 1), dev)

    def _update(self, u):
        """Update u of a call: the steps of the class's docstring, each a method of its own that a subclass overrides singly."""
        buf = self.buffer
        buf.sample()
        ddpg_inputs(buf._b_obs, buf._b_obs_, buf._b_act, central=self.central, out=(self._x_cur, self._x_next, self._x_pi))
        self._next_actions()
        self._critics_forward()
        self._head(u, buf.weights if self._prioritized else None)
        if self._prioritized:
            buf.update_priorities(self.critics[0].q, self.td)
        self._critics_step(u)
        self._actor_half(u)

    def _next_actions(self):
        """Step 3: the next state's actions into x_next."""
        _mlp_forward(_lib.load(), self._blob_ta, self.buffer._b_obs_, self._y4)
        ddpg_put_actions(self._y4, self._x_next, self.Do, self.k, central=self.central, own_only=False)

    def _critics_forward(self):
        """Steps 4 and 5: the target critics on x_next in order, then the critics on x_cur in order."""
        lib = _lib.load()
        for c in self.critics:
            _mlp_forward(lib, c.target_blob, self._x_next, self._yq4, c.q_next)
        for c in self.critics:
            _mlp_forward(lib, c.blob, self._x_cur, self._yq4, c.q)

    def _head(self, u, weight):
        """Step 6: the TD target, the critics' grad_out and the statistics of update u."""
        c, = self.critics
        td_head(c.q, c.q_next, self.buffer._b_rew, self.buffer._b_done, self.gamma, weight=weight, out=(c.g_q, self._g_pi, self.td, self.stats[u]),
                workspace=self._head_ws)

    def _critics_step(self, u, polyak=True):
        """Step 7: the critics' gradients in order, then ONE Adam step of them all; polyak: it carries their targets along."""
        lib, cs = _lib.load(), self.critics
        rows = [_mlp_grad(lib, c.buf, c.blob, self._x_cur, c.g_q, False) for c in cs]
        targets = dict(targets=[c.target for c in cs], target_blobs=[c.target_blob for c in cs]) if polyak else {}
        mlp_adam_step([c.net for c in cs], rows, [c.adam for c in cs], [c.blob for c in cs], self.hyper_critic, self.step_critic,
                      stats=self.step_stats_critic[u], workspace=self._adam_ws, **targets)

    def _actor_half(self, u):
        """Steps 8 to 10: the deterministic policy gradient through the stepped critic 1, the actor's step with its target."""
        lib, obs, c = _lib.load(), self.buffer._b_obs, self.critics[0]
        Do, k, central = self.Do, self.k, self.central
        _mlp_forward(lib, self._blob_a, obs, self._y4)
        ddpg_put_actions(self._y4, self._x_pi, Do, k, central=central, own_only=True)
        _mlp_grad(lib, c.buf, c.blob, self._x_pi, self._g_pi, False, c.buf["gx"])
        ddpg_action_grad(c.buf["gx"], Do, k, central=central, out=self._g_a4)
        row_a = _mlp_grad(lib, self._buf_a, self._blob_a, obs, self._g_a4, True)
        self._adam_one(self._actor_net, row_a, self.hyper_actor, self.step_actor, self.step_stats_actor[u])

    def set_lr(self, actor=None, critic=None):
        """The learning rates of the steps from now on, written to the hyper rows on the device (fills on the current stream: no host
        synchronisation); a captured update reads them at every replay.  None leaves a rate as it is."""
        for hyper, lr in ((self.hyper_actor, actor), (self.hyper_critic, critic)):
            if lr is not None:
                hyper[0].fill_(_hyper("lr", lr))
