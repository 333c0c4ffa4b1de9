"""QMIX for the discrete game on device (csrc/bsx_qmix_head.hip): the monotone mixing head between the fused MLP calls of two networks,
and the learner around it.

  qmix_members(nA, embed)               Mh, the member count of the mixer network of a team
  qmix_inputs                           the mixer's two inputs from a batch: every member reads the team's joint observation
  qmix_head                             the mix, its (double) Q-learning target and BOTH networks' grad_out, in one pass
  QMIXLearner(buffer, qnet, mixer, ...) QMIX of a team from its DeviceReplayBuffer; capture() makes it one graph

The Q network is dqn.py's: the StackedActor(nA, Do, 4) the rollout plays, Q_i(o, a) = q_scale * tanh row.  The mixer is a
StackedActor(Mh, nA Do, 4) whose tanh rows on the team's joint observation are the weights of the monotone mix (the hypernetwork of
Rashid et al. 2018), so its forward, backward, Adam step, Polyak target and packed blobs are the fused MLP kernels' own.  The ring, the
networks' records, capture(), sync() and publish() are ddpg.py's (_RingLearner), the Q network's half of the constructor and of an
update dqn.py's (_QLearner); qmix_head's argument check is ddpg.py's _head_args.
"""
from collections import namedtuple
from functools import partial

import torch

from .. import _lib
from .._args import _F32, _need, _workspace
from ..rollout import StackedActor
from ._common import _POSITIVE, _WEIGHT, _f32, _hyper, _ptr, _stream
from .adam import mlp_adam_step_workspace_bytes
from .ddpg import _head_args, _stacked_shape
from .dqn import _QLearner
from .mlp import _check_mlp, _mlp_forward, _mlp_grad

QmixHead = namedtuple("QmixHead", "g4 gh q td stats")
QMIX_STATS = ("n", "loss", "q_tot", "target", "abs_td", "done", "weight", "greedy")
EMBEDS = _lib.QMIX_EMBEDS
MAX_AGENTS = _lib.QMIX_MAX_AGENTS


def qmix_members(nA, embed):
    """Mh = nA m + 2 m + 1 with m = embed / 4: the members of the mixer of a team of nA agents (1 .. 4) at embedding width embed (4, 8
    or 16): nA m rows of W1, m of b1, m of w2 and one whose column 0 is b2.  Pure host arithmetic (`bsx_qmix_members` answers the same)."""
    nA, embed = int(nA), int(embed)
    if embed not in EMBEDS:
        raise ValueError(f"embed must be one of {EMBEDS}, got {embed!r}")
    if not 1 <= nA <= MAX_AGENTS:
        raise ValueError(f"the QMIX head mixes 1 .. {MAX_AGENTS} agents, got {nA}")
    m = embed // 4
    return nA * m + 2 * m + 1


def _joint_width(nA, Do):
    S = nA * Do
    if S > _lib.MLP_MAX_D:
        raise ValueError(f"the mixer reads the team's joint observation, {nA} x {Do} = {S} inputs: the fused MLP kernels take at most "
                         f"{_lib.MLP_MAX_D}")
    return S


def qmix_head_workspace_bytes(B, nA):
    """Bytes of the workspace qmix_head needs for B rows (td_head's at one element per row)."""
    return _lib.query_bytes("bsx_qmix_head_workspace_bytes", B, nA)


def qmix_inputs(obs, obs_next, members, *, out=None):
    """The mixer's two inputs from a sampled batch, in one launch (csrc/bsx_qmix_head.hip, `bsx_qmix_inputs`) -> (x_cur, x_next), each
    float32 [B, members, nA Do]: every member's row is the batch row's joint observation, obs[b].reshape(-1) / obs_next[b].reshape(-1),
    as bit copies.  obs, obs_next float32 [B, nA, Do], 1 <= nA <= 4 and nA Do <= 64; members in 1 .. 32 (qmix_members).  out: the two
    tensors to write into (nothing is allocated then)."""
    if not isinstance(obs, torch.Tensor) or obs.dim() != 3:
        raise ValueError("obs must be a float32 [B, nA, Do] tensor")
    if obs.device.type != "cuda":
        raise ValueError(f"qmix_inputs runs on the GPU: obs is on {obs.device}")
    (B, nA, Do), dev, Mh = obs.shape, obs.device, int(members)
    if not 1 <= B < 1 << 31 or not 1 <= nA <= MAX_AGENTS or not 1 <= Mh <= 2 * _lib.MAX_N:
        raise ValueError(f"1 <= B < 2^31, 1 .. {MAX_AGENTS} agents and 1 .. {2 * _lib.MAX_N} members are needed, got {B}, {nA} and {Mh}")
    S = _joint_width(nA, Do)
    need = partial(_need, dev=dev, anchor="obs")
    need(obs, "obs", (B, nA, Do), _F32)
    need(obs_next, "obs_next", (B, nA, Do), _F32)
    if out is None:
        out = tuple(torch.empty((B, Mh, S), dtype=torch.float32, device=dev) for _ in range(2))
    x_cur, x_next = out
    need(x_cur, "out x_cur", (B, Mh, S), _F32)
    need(x_next, "out x_next", (B, Mh, S), _F32)
    _lib.check(_lib.load().bsx_qmix_inputs(obs.data_ptr(), obs_next.data_ptr(), B, nA, Do, Mh, x_cur.data_ptr(), x_next.data_ptr(), _stream(dev)),
               "bsx_qmix_inputs")
    return x_cur, x_next


def qmix_head(y_cur, y_next_target, hy_cur, hy_next_target, act, rew, done, gamma, *, embed, q_scale, y_next_online=None, huber_delta=0.0,
              weight=None, out=None, workspace=None):
    """The monotone mix of a team's Q values, its (double) Q-learning target and the grad_out of BOTH networks, in one pass
    (csrc/bsx_qmix_head.hip, `bsx_qmix_head`; the exact contract, operation by operation, is written out in include/battlespace_hip.h)
    -> QmixHead(g4, gh, q, td, stats).

    y_cur, y_next_target, y_next_online, act, rew, done, gamma, q_scale, huber_delta: dqn_head's, with 1 <= nA <= 4.  hy_cur,
    hy_next_target float32 [B, Mh, 4], Mh = qmix_members(nA, embed): the ONLINE mixer's tanh rows on x_cur and the TARGET mixer's on
    x_next (bsx_mlp_forward's y on qmix_inputs' tensors).  In tanh units the rows are |.| -> W1 [nA][E], b1 [E], |.| -> w2 [E] and b2;
    per batch row, with u_i = y_cur[b, i][argmax4(act[b, i])],
        h_e = elu'(b1_e + sum_i u_i W1[i][e]),   Q_tot = q_scale (b2 + sum_e h_e w2_e),   elu'(x) = x for x > 0, else x / (1 - x)
    -- monotone in every u_i --, the target y = sum_i rew[b, i] + gamma (every agent done ? 0 : Q_tot' of the greedy next values on the
    target rows, a finished agent's value 0), d = Q_tot - y clipped to [-huber_delta, huber_delta] where huber_delta > 0, w =
    weight[b, 0] or 1.  g4 float32 [B, nA, 4] and gh float32 [B, Mh, 4] are mlp_grad's grad_out (squash=True) of the Q network and of
    the mixer for mean_b w l(Q_tot - y).  q = Q_tot and td = y in every one of the nA columns (what update_priorities takes).  stats
    f64 [8] on the device in the order of learner.QMIX_STATS: n = B, then means over the B rows; `greedy` is the share of replayed
    actions that are the online network's greedy one.  Deterministic; two launches on the current stream, no host synchronisation.
    out: optional (g4, gh, q, td or None, stats) to write into and workspace (at least qmix_head_workspace_bytes(B, nA) bytes, 8-byte
    aligned) -- pass both and nothing is allocated (a captured graph)."""
    embed = int(embed)
    if embed not in EMBEDS:
        raise ValueError(f"embed must be one of {EMBEDS}, got {embed!r}")
    q_scale, huber_delta = _hyper("q_scale", q_scale, _POSITIVE), _hyper("huber_delta", huber_delta, _WEIGHT)
    if isinstance(y_cur, torch.Tensor) and y_cur.dim() == 3 and y_cur.shape[1] > MAX_AGENTS:
        raise ValueError(f"the QMIX head mixes 1 .. {MAX_AGENTS} agents, got {y_cur.shape[1]}")
    gh = None
    if out is not None:
        if len(out) != 5:
            raise ValueError("out must be (g4, gh, q, td or None, stats)")
        gh, out = out[1], (out[0],) + tuple(out[2:])
    rows4 = ((y_cur, "y_cur"), (y_next_target, "y_next_target"), (y_next_online, "y_next_online"), (act, "act"))
    B, nA, dev, gamma, (g4, q, td, stats), workspace = _head_args("qmix_head", ((rew, "rew"),), done, gamma, weight, ("g4",), out, workspace,
                                                                 rows4=rows4, values=("q",))
    Mh = qmix_members(nA, embed)
    need = partial(_need, dev=dev, anchor="y_cur")
    need(hy_cur, "hy_cur", (B, Mh, 4), _F32)
    need(hy_next_target, "hy_next_target", (B, Mh, 4), _F32)
    if gh is None:
        gh = torch.empty((B, Mh, 4), dtype=torch.float32, device=dev)
    need(gh, "out gh", (B, Mh, 4), _F32)
    io = _lib.BsxQmixIo(y_cur.data_ptr(), _ptr(y_next_online), y_next_target.data_ptr(), hy_cur.data_ptr(), hy_next_target.data_ptr(),
                        act.data_ptr(), rew.data_ptr(), done.data_ptr(), _ptr(weight), g4.data_ptr(), gh.data_ptr(), q.data_ptr(), _ptr(td))
    _lib.check(_lib.load().bsx_qmix_head(_lib.ctypes.byref(io), B, nA, embed, gamma, q_scale, huber_delta, int(y_next_online is not None),
                                         workspace.data_ptr(), stats.data_ptr(), _stream(dev)), "bsx_qmix_head")
    return QmixHead(g4, gh, q, td, stats)


class QMIXLearner(_QLearner):
    """QMIX of a team for the discrete game from its replay ring, on device (Rashid et al. 2018): per-plane Q networks, a monotone
    mixing network whose weights a hypernetwork makes from the team's joint observation, double Q, soft target networks, Adam.  What
    DQNLearner(mix="vdn") cannot represent -- a team value that is not a sum of per-plane terms: a base that falls to combined fire, a
    kill worth more while the partner lives -- this mix can, and each plane still plays its own arg-max.

        buf = PrioritizedReplayBuffer(1_000_000, 512, env.possible_red, env.obs_size, env.obs_size * n, 4, seed=0)
        learner = QMIXLearner(buf, qnet, embed=8, q_scale=20.0)        # qnet: the StackedActor(n, obs_size, 4) the rollout plays
        learner.capture()
        while training:
            ro.run(); buf.append_rollout(ro, range(n))
            stats = learner.update()                      # f64 [updates, 8] on the device, columns in the order of learner.QMIX_STATS
            learner.publish(ro, range(n))                 # the rollout plays the updated Q network; the mixer stays with the learner

    The Q network is DQNLearner's: Q_i(o, a) = q_scale * tanh-row[i][a], the learner's greedy action and the published rollout's action
    the same bits.  The mixer is a StackedActor(Mh, nA Do, 4), Mh = qmix_members(nA, embed) (one is made if none is given): its tanh
    rows are the mix's weights in tanh units, so |Q_tot| <= q_scale (1 + embed); choose q_scale >= r_max / (1 - gamma) as for DQN.
    Execution stays decentralised: publish() copies the Q network alone.  The behaviour policy is the rollout's, as for DQN:
    PolicyRollout(epsilon=EpsilonSchedule(start, end, steps)) is the paper's annealed epsilon-greedy.  Limits: nA <= 4, nA Do <= 64 (4v4: 56), embed 4, 8 or 16.

    One update, on the current stream, with cached buffers and no host synchronisation:
       1. buffer.sample()                                          the batch, drawn on the device
       2. online network on obs -> y_cur
       3. double=True: online network on obs_next -> y_next_online (double=False: no launch)
       4. target network on obs_next -> y_next_target
       5. qmix_inputs                                              x_cur, x_next: the joint observation for every mixer member
       6. mixer on x_cur -> hy_cur;   7. target mixer on x_next -> hy_next_target
       8. qmix_head                                                Q_tot, y, g4, gh, the statistics
          (a PrioritizedReplayBuffer: with weight = buffer.weights, then buffer.update_priorities(q, y): every column holds the row's
          |Q_tot - y|)
       9. mlp_grad(squash=True) of the Q network on obs with g4;  10. mlp_grad(squash=True) of the mixer on x_cur with gh
      11. ONE mlp_adam_step of the Q network with its Polyak target;  12. ONE of the mixer with its
    Clipping (max_grad_norm) is per network, as in DDPGLearner's two steps.

    buffer: a DeviceReplayBuffer with n_actions == 4.  The learner owns deep copies of both networks as targets (`target_qnet`,
    `target_mixer`), the four packed blobs, two AdamStates (`adam`, `adam_mixer`), ONE hyper row `hyper` (adam_hyper with tau), two step
    counters (`step`, `step_mixer`) and the statistics: `stats` f64 [updates, 8] (QMIX_STATS), `step_stats` and `step_stats_mixer` f64
    [updates, 4] (ADAM_STATS).  update() runs `updates` updates and returns `stats`; capture() records them as ONE graph, the ring's
    draw included, and leaves every bit as it was; set_lr writes the device hyper row; sync() re-packs all four blobs after an outside
    edit.  Nothing is allocated after construction.  n-step targets need nothing here: fill the ring through replay.NStepAppender and
    give the learner gamma=app.bootstrap_gamma."""

    def __init__(self, buffer, qnet, mixer=None, *, embed=8, double=True, q_scale, huber_delta=0.0, gamma=0.95, tau=0.01, lr=1e-3,
                 betas=(0.9, 0.999), eps=1e-8, max_grad_norm=None, updates=1):
        mgn = self._q_args(buffer, double=double, q_scale=q_scale, huber_delta=huber_delta, gamma=gamma, updates=updates, max_grad_norm=max_grad_norm)
        nA, Do, B, dev = self.nA, self.Do, self.B, buffer.actor_states.device
        Mh = qmix_members(nA, embed)                                # refuses the embed, then the team
        S = _joint_width(nA, Do)
        self.embed, self.members, self.S = int(embed), Mh, S
        if mixer is None:
            mixer = StackedActor(Mh, S, 4, device=dev)
        _stacked_shape(qnet, "qnet", (nA, Do, 4), f" and embed={int(embed)}")
        _stacked_shape(mixer, "mixer", (Mh, S, 4), f" and embed={int(embed)}")
        self._q_state(qnet, mgn, tau=tau, lr=lr, betas=betas, eps=eps)
        f = _f32(torch.zeros, dev)
        self._x_cur, self._x_next = f(B, Mh, S), f(B, Mh, S)
        _check_mlp(mixer, self._x_cur, True, type(self).__name__)
        self._mixer_net = self._net(mixer, S, members=Mh)
        self.critics.append(self._mixer_net)                        # the second network sync() and the state list run over
        self.mixer, self.target_mixer, self._blob_m, self._blob_tm, self.adam_mixer, self._buf_m = self._mixer_net[:6]
        self.step_mixer = torch.zeros(1, dtype=torch.int64, device=dev)
        self.step_stats_mixer = torch.zeros((self.updates, 4), dtype=torch.float64, device=dev)
        self._steps.append((self.step_mixer, self.step_stats_mixer))
        self._hy_cur, self._hy_tg, self._gh = (f(B, Mh, 4) for _ in range(3))
        self._head_ws = _workspace(None, qmix_head_workspace_bytes(B, nA), dev)
        self._adam_ws = _workspace(None, max(mlp_adam_step_workspace_bytes(nA, 1), mlp_adam_step_workspace_bytes(Mh, 1)), dev)

    def _update(self, u):
        """Update u of a call: the steps of the class's docstring."""
        buf = self.buffer
        buf.sample()
        lib, y_on, weight = self._q_forwards()
        qmix_inputs(buf._b_obs, buf._b_obs_, self.members, out=(self._x_cur, self._x_next))
        _mlp_forward(lib, self._blob_m, self._x_cur, self._hy_cur)
        _mlp_forward(lib, self._blob_tm, self._x_next, self._hy_tg)
        qmix_head(self._y_cur, self._y_tg, self._hy_cur, self._hy_tg, buf._b_act, buf._b_rew, buf._b_done, self.gamma, embed=self.embed,
                  q_scale=self.q_scale, y_next_online=y_on, huber_delta=self.huber_delta, weight=weight,
                  out=(self._g4, self._gh, self.q, self.td, self.stats[u]), workspace=self._head_ws)
        row_q = self._after_head(lib)
        row_m = _mlp_grad(lib, self._buf_m, self._blob_m, self._x_cur, self._gh, True)
        self._adam_one(self._actor_net, row_q, self.hyper, self.step, self.step_stats[u])
        self._adam_one(self._mixer_net, row_m, self.hyper, self.step_mixer, self.step_stats_mixer[u])
