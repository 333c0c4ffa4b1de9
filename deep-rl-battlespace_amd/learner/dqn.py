"""Q-learning for the discrete game on device (csrc/bsx_dqn_head.hip): the head between the fused MLP calls, and the learner around it.

  dqn_head                              the (double) Q-learning target, independent or VDN-mixed, and the network's grad_out, in one pass
  DQNLearner(buffer, qnet, ...)         independent DQN or VDN of a team from its DeviceReplayBuffer; capture() makes it one graph
  _QLearner                             what DQNLearner and qmix.QMIXLearner share: the Q network's half of the constructor and of an update

The Q network of a team is the network its rollout plays, a StackedActor(nA, Do, 4), with Q_i(o, a) = q_scale * y4[i][a] on the
tanh-squashed row of bsx_mlp_forward: the learner's greedy action and the action a published rollout plays are the same bits.  The
ring, the networks' records, capture(), sync() and publish() are ddpg.py's (_RingLearner); dqn_head's argument check is its _head_args.
"""
from collections import namedtuple

import torch

from .. import _lib
from .._args import _workspace
from ._common import _POSITIVE, _WEIGHT, _f32, _hyper, _ptr, _stream
from .adam import adam_hyper, mlp_adam_step_workspace_bytes
from .ddpg import _head_args, _RingLearner, _stacked_shape
from .mlp import _check_mlp, _mlp_forward, _mlp_grad

DqnHead = namedtuple("DqnHead", "g4 q td stats")
DQN_STATS = ("n", "loss", "q", "target", "abs_td", "done", "weight", "greedy")
MIXES = ("independent", "vdn")


def _mix(mix):
    if mix not in MIXES:
        raise ValueError(f"mix must be 'independent' or 'vdn', got {mix!r}")
    return MIXES.index(mix)


def dqn_head_workspace_bytes(B, nA):
    """Bytes of the workspace dqn_head needs for B rows of nA agents (td_head's)."""
    return _lib.query_bytes("bsx_dqn_head_workspace_bytes", B, nA)


def dqn_head(y_cur, y_next_target, act, rew, done, gamma, *, q_scale, y_next_online=None, mix="independent", huber_delta=0.0, weight=None,
             out=None, workspace=None):
    """The target of (double) Q-learning and the Q network's grad_out, in one pass (csrc/bsx_dqn_head.hip, `bsx_dqn_head`; the exact
    contract is written out in include/battlespace_hip.h) -> DqnHead(g4, q, td, stats).

    y_cur, y_next_target float32 [B, nA, 4]: the online network's tanh rows on obs and the target network's on obs_next
    (bsx_mlp_forward's y); y_next_online: the online network's on obs_next -- given, it picks the next action (double Q), else the target
    rows pick it themselves.  act float32 [B, nA, 4]: the replayed score rows (the ring's act, n_actions = 4); rew float32 [B, nA]; done
    uint8 or bool [B, nA]; weight float32 [B, nA] or None; gamma in [0, 1]; q_scale > 0; huber_delta >= 0 (0: the squared error).  With
    argmax4 the step kernel's choice (the first maximum; a NaN counts as the maximum), per element a = argmax4(act), a' = argmax4 of the
    picking rows, qn = done ? 0 : q_scale y_next_target[a'], qc = q_scale y_cur[a]; mix="independent": Q = qc, y = fmaf(gamma, qn, rew),
    w = weight; mix="vdn": Q, the next value and the reward are float32 sums over the row's agents in agent order, w = weight[:, 0], and
    every agent of the row carries the row's Q, y and w.  d = Q - y, clipped to [-huber_delta, huber_delta] where huber_delta > 0;
    g4[..., a] = ((w d) float(2 / B)) q_scale and +0 in the other three columns: mlp_grad's grad_out (squash=True) for the sum over agents
    of mean_b w l(Q_i - y_i), or for mean_b w l(Q_tot - y_tot) under VDN.  q = Q, td = y.  stats f64 [8] on the device in the order of
    learner.DQN_STATS: means over the B nA elements; `greedy` is the share of replayed actions that are the online network's greedy one.
    Q is bounded by q_scale: choose q_scale >= r_max / (1 - gamma); a target beyond q_scale cannot be reached.  Deterministic; two
    launches on the current stream, no host synchronisation.  out: optional (g4, q, td or None, stats) to write into and workspace (at
    least dqn_head_workspace_bytes(B, nA) bytes, 8-byte aligned) -- pass both and nothing is allocated (a captured graph)."""
    m = _mix(mix)
    q_scale, huber_delta = _hyper("q_scale", q_scale, _POSITIVE), _hyper("huber_delta", huber_delta, _WEIGHT)
    rows4 = ((y_cur, "y_cur"), (y_next_target, "y_next_target"), (y_next_online, "y_next_online"), (act, "act"))
    B, nA, dev, gamma, (g4, q, td, stats), workspace = _head_args("dqn_head", ((rew, "rew"),), done, gamma, weight, ("g4",), out, workspace,
                                                                 rows4=rows4, values=("q",))
    io = _lib.BsxDqnIo(y_cur.data_ptr(), _ptr(y_next_online), y_next_target.data_ptr(), act.data_ptr(), rew.data_ptr(), done.data_ptr(),
                       _ptr(weight), g4.data_ptr(), q.data_ptr(), _ptr(td))
    _lib.check(_lib.load().bsx_dqn_head(_lib.ctypes.byref(io), B, nA, gamma, q_scale, huber_delta, int(y_next_online is not None), m,
                                        workspace.data_ptr(), stats.data_ptr(), _stream(dev)), "bsx_dqn_head")
    return DqnHead(g4, q, td, stats)


class _QLearner(_RingLearner):
    """What DQNLearner and qmix.QMIXLearner share, and no learner on its own.  The constructor in its two halves, between which a
    subclass refuses the shapes of its networks (every shape refusal comes before the first look at a network's tensors): `_q_args`, the
    refusals and hypers that need no network, and `_q_state`, the Q network a rollout plays as the record `_actor_net` with its public
    aliases, ONE hyper row, the Q network's step counter and statistics and the head's row buffers.  Of an update: the three forwards of
    the Q network and what follows the head up to the Q network's gradient; and set_lr.  A subclass adds its head's workspace
    `_head_ws` (and, with more networks, their records to `critics` and their pairs to `_steps`) and writes `_update(u)`."""

    def _q_args(self, buffer, *, double, q_scale, huber_delta, gamma, updates, max_grad_norm):
        """-> max_grad_norm as adam_hyper takes it; sets the hypers and `nA`, `Do`, `k`, `B`."""
        mgn = self._ring(buffer, gamma, updates, max_grad_norm)
        self.double = bool(double)
        self.q_scale, self.huber_delta = _hyper("q_scale", q_scale, _POSITIVE), _hyper("huber_delta", huber_delta, _WEIGHT)
        if buffer.n_actions != 4:
            raise ValueError(f"{type(self).__name__} learns the discrete game: the ring must keep the four action scores (n_actions == 4), "
                             f"got {buffer.n_actions}")
        self.nA, self.Do, self.k, self.B = buffer.n_agents, buffer.actor_states.shape[2], 4, buffer.batch_size
        return mgn

    def _q_state(self, qnet, mgn, *, tau, lr, betas, eps):
        """qnet: of the shape the subclass has checked (_stacked_shape)."""
        buffer, nA, Do, B = self.buffer, self.nA, self.Do, self.B
        dev = buffer.actor_states.device
        _check_mlp(qnet, buffer._b_obs, True, type(self).__name__)
        self.critics = []
        self._actor_net = self._net(qnet, Do)
        self.qnet, self.target_qnet, self._blob_q, self._blob_tq, self.adam, self._buf_q = self._actor_net[:6]
        self.hyper = adam_hyper(lr, betas, eps, mgn, dev, tau)
        self.step = torch.zeros(1, dtype=torch.int64, device=dev)
        self.stats = torch.zeros((self.updates, 8), dtype=torch.float64, device=dev)
        self.step_stats = torch.zeros((self.updates, 4), dtype=torch.float64, device=dev)
        self._steps = [(self.step, self.step_stats)]
        f = _f32(torch.zeros, dev)
        self._y_cur, self._y_on, self._y_tg, self._g4 = (f(B, nA, 4) for _ in range(4))
        self.q, self.td = f(B, nA), f(B, nA)
        self._adam_ws = _workspace(None, mlp_adam_step_workspace_bytes(nA, 1), dev)

    def _q_forwards(self):
        """After the draw: the online network on obs -> y_cur, double=True: on obs_next -> y_next_online (double=False: no launch), the
        target network on obs_next -> y_next_target.  -> (the library, y_next_online or None: what the head takes, the batch's weight or None)"""
        lib, buf = _lib.load(), self.buffer
        _mlp_forward(lib, self._blob_q, buf._b_obs, self._y_cur)
        if self.double:
            _mlp_forward(lib, self._blob_q, buf._b_obs_, self._y_on)
        _mlp_forward(lib, self._blob_tq, buf._b_obs_, self._y_tg)
        return lib, self._y_on if self.double else None, buf.weights if self._prioritized else None

    def _after_head(self, lib):
        """After the head: a prioritised ring's new priorities from (q, y), then the Q network's gradient from g4 -> its row."""
        if self._prioritized:
            self.buffer.update_priorities(self.q, self.td)
        return _mlp_grad(lib, self._buf_q, self._blob_q, self.buffer._b_obs, self._g4, True)

    def set_lr(self, lr):
        """The learning rate of the steps from now on -- of every network the learner steps --, written to the hyper row on the device (a
        fill on the current stream: no host synchronisation); a captured update reads it at every replay."""
        self.hyper[0].fill_(_hyper("lr", lr))


class DQNLearner(_QLearner):
    """Q-learning of a team for the discrete game from its replay ring, on device: independent DQN per agent (Mnih et al. 2015) or the
    value-decomposition mix of the team (mix="vdn"; Sunehag et al. 2018), double Q (van Hasselt et al. 2016), a soft target network, Adam.

        buf = PrioritizedReplayBuffer(1_000_000, 512, env.possible_red, env.obs_size, env.obs_size * n, 4, seed=0)
        learner = DQNLearner(buf, qnet, mix="vdn", q_scale=20.0)       # qnet: the StackedActor(n, obs_size, 4) the rollout plays
        learner.capture()
        while training:
            ro.run(); buf.append_rollout(ro, range(n))
            stats = learner.update()                      # f64 [updates, 8] on the device, columns in the order of learner.DQN_STATS
            learner.publish(ro, range(n))                 # the rollout plays the updated network

    The Q network is the network the rollout plays and Q_i(o, a) = q_scale * tanh-row[i][a]: bsx_mlp_forward is the rollout's float32
    kernel and the step kernel takes its arg-max over the same tanh row, so the learner's greedy action and the published rollout's
    action are the same bits, ties and saturation included.  Q is bounded by q_scale: choose q_scale >= r_max / (1 - gamma); a target
    beyond q_scale cannot be reached (the tanh saturates and the gradient fades).  The behaviour policy is the rollout's: the
    algorithm's own is annealed epsilon-greedy, PolicyRollout(epsilon=EpsilonSchedule(start, end, steps)) on the rollout that plays the
    published network (a random row goes out one-hot, and the head replays it like any other); noise_std, ou_scale or
    sample="categorical" with a temperature remain.

    One update, on the current stream, with cached buffers and no host synchronisation:
       1. buffer.sample()                                          the batch, drawn on the device
       2. online network on obs -> y_cur
       3. double=True: online network on obs_next -> y_next_online (double=False: no launch)
       4. target network on obs_next -> y_next_target
       5. dqn_head                                                 y, g4, the statistics
          (a PrioritizedReplayBuffer: with weight = buffer.weights, then buffer.update_priorities(q, y); under VDN every column holds the
          row's |Q_tot - y_tot|)
       6. mlp_grad(squash=True, input_grad=False) of the network on obs with g4
       7. ONE mlp_adam_step with the Polyak target and both blobs

    buffer: a DeviceReplayBuffer with n_actions == 4 (the ring keeps the score rows the step kernel arg-maxed); its n_agents and
    observation size give nA and Do, its batch_size B.  qnet: a StackedActor(nA, Do, 4) on the buffer's device.  The learner owns a deep
    copy as the target (`target_qnet`), both packed blobs, the AdamState `adam`, the hyper row `hyper` (adam_hyper with tau), the step
    counter `step`, and the statistics: `stats` f64 [updates, 8] (DQN_STATS) and `step_stats` f64 [updates, 4] (ADAM_STATS).  update()
    runs `updates` updates and returns `stats`; capture() records them as ONE graph, the ring's draw included, and leaves every bit as it
    was; set_lr writes the device hyper row; sync() re-packs both blobs after an outside edit; publish copies the network into a rollout.
    n-step targets need nothing here: fill the ring through replay.NStepAppender and give the learner gamma=app.bootstrap_gamma, the
    appender's gamma^n; step 5 is then the n-step target."""

    def __init__(self, buffer, qnet, *, mix="independent", double=True, q_scale, huber_delta=0.0, gamma=0.95, tau=0.01, lr=1e-3,
                 betas=(0.9, 0.999), eps=1e-8, max_grad_norm=None, updates=1):
        self.mix, self._mix = mix, _mix(mix)
        mgn = self._q_args(buffer, double=double, q_scale=q_scale, huber_delta=huber_delta, gamma=gamma, updates=updates, max_grad_norm=max_grad_norm)
        _stacked_shape(qnet, "qnet", (self.nA, self.Do, 4))
        self._q_state(qnet, mgn, tau=tau, lr=lr, betas=betas, eps=eps)
        self._head_ws = _workspace(None, dqn_head_workspace_bytes(self.B, self.nA), self.hyper.device)

    def _update(self, u):
        """Update u of a call: the steps of the class's docstring."""
        buf = self.buffer
        buf.sample()
        lib, y_on, weight = self._q_forwards()
        dqn_head(self._y_cur, self._y_tg, buf._b_act, buf._b_rew, buf._b_done, self.gamma, q_scale=self.q_scale, y_next_online=y_on, mix=self.mix,
                 huber_delta=self.huber_delta, weight=weight, out=(self._g4, self.q, self.td, self.stats[u]), workspace=self._head_ws)
        self._adam_one(self._actor_net, self._after_head(lib), self.hyper, self.step, self.step_stats[u])
