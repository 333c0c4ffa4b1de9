"""The TD3 / MATD3 update on device (csrc/bsx_td3_head.hip): what it adds to ddpg.py's calls, and the learner around it.

  td3_smooth_actions, td3_head                  target policy smoothing into x_next, the TD head of two critics
  TD3Learner(buffer, actor, critic=None, critic2=None, ...)   twin critics, smoothed targets, a delayed actor and target step; one graph

DDPGLearner's update is a sequence of steps over a list of critics (ddpg.py).  _TwinCriticLearner here puts a second critic on that list --
the one place TD3Learner and learner.SACLearner get theirs from -- and TD3Learner overrides the steps that are TD3's: the next actions, the
head, and when the targets and the actor move.  td3_head's argument check is ddpg.py's _head_args, td_head's and sac_head's too.
"""
from collections import namedtuple
from functools import partial

import torch

from .. import _lib
from .._args import _F32, _need, _workspace
from ..rollout import StackedActor
from ._common import _U64, _WEIGHT, _hyper, _int64_word, _ptr, _stream
from .adam import mlp_adam_step_workspace_bytes
from .ddpg import DDPGLearner, _batch_rows, _critic_width, _head_args, _stacked_shape
from .mlp import _check_mlp, _mlp_forward

Td3Head = namedtuple("Td3Head", "g_q1 g_q2 g_pi td stats")
TD3_STATS = ("n", "critic_loss", "q", "target", "abs_td", "done", "weight", "q_gap")


def td3_smooth_actions(y4, x, obs_len, n_actions, *, sigma, clip, seed, seq=0, seq_base=None, z=None, central=True):
    """Target policy smoothing, in one launch (csrc/bsx_td3_head.hip, `bsx_td3_smooth_actions`; include/battlespace_hip.h) -> x.

    y4 float32 [B, nA, 4]: the target actors' output rows; x float32 [B, nA, Dc]: the critic input x_next.  Per (b, j) and action column
    c < n_actions, a' = clamp(y4[b, j, c] + clamp(sigma z[c], -clip, clip), -1, 1), every operation one float32 rounding, a NaN stays a
    NaN; a' goes where ddpg_put_actions(own_only=False) writes: slot j of every row (b, i) with central=True, the row's own action
    columns otherwise.  The noise is keyed by (b, j) alone: the nA rows of b hold the same bits.  z: float32 [B, nA, 4], the normals
    (tests); without it they are the project's Philox normals under (seed, seq + seq_base, b nA + j) and a salt of their own.  seq_base:
    an int64 device word read on the device (a captured graph draws fresh noise once the caller advances it), or None.  sigma, clip >= 0.
    Nothing else of x is written."""
    B, nA, dev = _batch_rows(y4, "y4")
    Do, k = int(obs_len), int(n_actions)
    Dc = _critic_width(nA, Do, k, central)
    sigma, clip = _hyper("sigma", sigma, _WEIGHT), _hyper("clip", clip, _WEIGHT)
    need = partial(_need, dev=dev, anchor="y4")
    need(y4, "y4", (B, nA, 4), _F32)
    need(x, "x", (B, nA, Dc), _F32)
    if z is not None:
        need(z, "z", (B, nA, 4), _F32)
    if seq_base is not None:
        _int64_word(seq_base, "seq_base", dev, "y4")
    _lib.check(_lib.load().bsx_td3_smooth_actions(y4.data_ptr(), B, nA, Do, k, int(bool(central)), sigma, clip, int(seed) & _U64, int(seq) & _U64,
                                                  _ptr(seq_base), _ptr(z), x.data_ptr(), _stream(dev)), "bsx_td3_smooth_actions")
    return x


def td3_head_workspace_bytes(B, nA):
    """Bytes of the workspace td3_head needs for B rows of nA agents."""
    return _lib.query_bytes("bsx_td3_head_workspace_bytes", B, nA)


def td3_head(q1, q2, q1_next, q2_next, rew, done, gamma, *, weight=None, out=None, workspace=None):
    """The TD target of clipped double-Q learning and the three grad_out tensors of a TD3 update, in one pass (csrc/bsx_td3_head.hip,
    `bsx_td3_head`; the exact contract is written out in include/battlespace_hip.h) -> Td3Head(g_q1, g_q2, g_pi, td, stats).

    q1, q2, q1_next, q2_next, rew float32 [B, nA]: the two critics on x_cur, the two target critics on x_next (raw heads) and the rewards;
    done uint8 or bool [B, nA]; weight float32 [B, nA] or None; gamma in [0, 1].  Per element m = min(q1_next, q2_next) (a NaN in either
    is a NaN), y = fmaf(gamma, done ? 0 : m, rew), d_i = q_i - y;  g_q1[..., 0] = (w d1) float(2 / B) and g_q2[..., 0] = (w d2)
    float(2 / B): the critics' grad_out (squash=False) for the sum over agents of mean_b w ((Q1 - y)^2 + (Q2 - y)^2);  g_pi[..., 0] =
    -(w float(1 / B)): the seed of critic 1's input-gradient pass (the actor reads critic 1 alone);  td = y.  Columns 1 .. 3 are +0.
    With q2 = q1 and q2_next = q1_next, g_q1, g_pi and td are td_head's bits.  stats f64 [8] on the device in the order of
    learner.TD3_STATS: means over the B nA elements.  Deterministic; two launches on the current stream, no host synchronisation.
    out: optional (g_q1, g_q2, g_pi, td or None, stats) to write into and workspace (at least td3_head_workspace_bytes(B, nA) bytes,
    8-byte aligned) -- pass both and nothing is allocated (a captured graph)."""
    rows = ((q1, "q1"), (q2, "q2"), (q1_next, "q1_next"), (q2_next, "q2_next"), (rew, "rew"))
    B, nA, dev, gamma, (g_q1, g_q2, g_pi, td, stats), workspace = _head_args("td3_head", rows, done, gamma, weight, ("g_q1", "g_q2", "g_pi"), out,
                                                                             workspace)
    io = _lib.BsxTd3Io(q1.data_ptr(), q2.data_ptr(), q1_next.data_ptr(), q2_next.data_ptr(), rew.data_ptr(), done.data_ptr(), _ptr(weight),
                       g_q1.data_ptr(), g_q2.data_ptr(), g_pi.data_ptr(), _ptr(td))
    _lib.check(_lib.load().bsx_td3_head(_lib.ctypes.byref(io), B, nA, gamma, workspace.data_ptr(), stats.data_ptr(), _stream(dev)), "bsx_td3_head")
    return Td3Head(g_q1, g_q2, g_pi, td, stats)


class _TwinCriticLearner(DDPGLearner):
    """DDPGLearner with a second critic: what TD3Learner and SACLearner share, and no learner on its own (it has no head for two critics).
    critic2: a second StackedActor(nA, Dc, 1), not `critic` itself; one is made if none is given.  On top of DDPGLearner's state it owns
    `critic2`, `target_critic2`, their blobs `_blob_c2` and `_blob_tc2`, `adam_critic2` -- the second record of `critics`, so the
    forwards, the gradients, the joint Adam step, capture() and sync() cover both -- and `_noise_draws`, the sequence word of the
    subclass's draws (with `seed` their key), advanced by one per drawing call.  gx2: critic 2 also gives input gradients."""

    def __init__(self, buffer, actor, critic, critic2, *, seed, gx2, critic_input, **kw):
        if critic2 is not None and critic2 is critic:
            raise ValueError("critic2 is critic itself: the second critic is a network of its own")
        self.seed = int(seed)
        super().__init__(buffer, actor, critic, critic_input=critic_input, **kw)
        nA, Dc, dev = self.nA, self.Dc, self._x_cur.device
        if critic2 is None:
            critic2 = StackedActor(nA, Dc, 1, device=dev)
        _stacked_shape(critic2, "critic2", (nA, Dc, 1), f" and critic_input={critic_input!r}")
        _check_mlp(critic2, self._x_cur, False, type(self).__name__)
        self.critic2, self.target_critic2, self._blob_c2, self._blob_tc2, self.adam_critic2 = self._net(critic2, Dc, critic=True, gx=gx2)[:5]
        self._noise_draws = torch.zeros(1, dtype=torch.int64, device=dev)
        self._adam_ws = _workspace(None, max(mlp_adam_step_workspace_bytes(nA, 1), mlp_adam_step_workspace_bytes(nA, 2)), dev)

    def _state(self):
        return super()._state() + [self._noise_draws]


class TD3Learner(_TwinCriticLearner):
    """The MATD3 update of a team from its replay ring, on device (Fujimoto et al. 2018; Ackermann et al. 2019 for the multi-agent form):
    DDPGLearner's networks, ring and critic inputs with TD3's three pieces -- a second critic and a target that bootstraps from the
    smaller of the two target critics; clipped Gaussian noise on the target actors' actions; the actor and ALL target networks stepped
    once per `policy_delay` critic steps.

        learner = TD3Learner(buf, actor, updates=2, policy_delay=2)     # critics StackedActor(n, Dc, 1) are made, each with its own initialisation
        learner.capture()
        while training:
            ro.run(); buf.append_rollout(ro, range(n))
            stats = learner.update()                      # f64 [updates, 8] on the device, columns in the order of learner.TD3_STATS
            learner.publish(ro, range(n))

    Update u of a call, on the current stream, with cached buffers and no host synchronisation:
       1. buffer.sample(), ddpg_inputs
       2. target actor on obs_next, td3_smooth_actions             a' = clamp(pi'(o') + clamp(target_noise z, -noise_clip, noise_clip), -1, 1)
          into x_next, keyed by `seed` and the device word `_noise_draws`, which then advances by 1 (target_noise = 0: the plain
          ddpg_put_actions(own_only=False), and the word stays)
       3. both target critics on x_next, both critics on x_cur
       4. td3_head                                                 y = r + gamma (1 - done) min(q1_next, q2_next), g_q1, g_q2, g_pi, the statistics
          (a PrioritizedReplayBuffer: with weight = buffer.weights, then buffer.update_priorities(q1, y))
       5. mlp_grad of critic 1 with g_q1 and of critic 2 with g_q2, then ONE mlp_adam_step of both: one norm over both, one step counter;
          it carries the critics' Polyak targets only when (u + 1) % policy_delay == 0
       6. only then: actor on obs, ddpg_put_actions(own_only=True), mlp_grad of the STEPPED critic 1 on x_pi with g_pi -> grad_x,
          ddpg_action_grad, mlp_grad of the actor, mlp_adam_step of the actor with its target.

    buffer, actor, critic, critic_input, gamma, tau, the learning rates, betas, eps, max_grad_norm: DDPGLearner's.  critic2: a second
    StackedActor(nA, Dc, 1), not `critic` itself; one is made if none is given.  updates must be a multiple of policy_delay >= 1, so that
    a captured call keeps the schedule from replay to replay.  target_noise (sigma) and noise_clip are >= 0.  On top of DDPGLearner's
    state the learner owns `target_critic2`, two more blobs, `adam_critic2` and `_noise_draws`; `stats` is f64 [updates, 8] in the order
    of TD3_STATS, `step_stats_critic` holds the joint step of both critics, and the rows of `step_stats_actor` of updates without an
    actor step stay as they were.  update(), capture(), set_lr(), sync() (six blobs) and publish() are DDPGLearner's, over the two
    critics of _TwinCriticLearner; the steps of an update that are TD3's own are the methods below.  Parameter
    sharing is not here.  On a ring filled through replay.NStepAppender the head's target is the n-step one when the learner is given
    gamma=app.bootstrap_gamma."""

    def __init__(self, buffer, actor, critic=None, critic2=None, *, critic_input="central", gamma=0.95, tau=0.01, lr_actor=1e-3,
                 lr_critic=1e-3, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=None, updates=2, policy_delay=2, target_noise=0.2,
                 noise_clip=0.5, seed=0):
        if isinstance(policy_delay, bool) or not isinstance(policy_delay, int) or policy_delay < 1:
            raise ValueError(f"policy_delay must be an int >= 1, got {policy_delay!r}")
        if int(updates) < 1 or int(updates) % policy_delay:
            raise ValueError(f"updates must be a multiple of policy_delay = {policy_delay} (a call keeps the schedule), got {updates!r}")
        self.policy_delay = policy_delay
        self.target_noise, self.noise_clip = _hyper("target_noise", target_noise, _WEIGHT), _hyper("noise_clip", noise_clip, _WEIGHT)
        super().__init__(buffer, actor, critic, critic2, seed=seed, gx2=False, critic_input=critic_input, gamma=gamma, tau=tau, lr_actor=lr_actor,
                         lr_critic=lr_critic, betas=betas, eps=eps, max_grad_norm=max_grad_norm, updates=updates)

    def _next_actions(self):
        """Step 2: DDPGLearner's without noise; else the smoothed actions, and the sequence word advances."""
        if not self.target_noise > 0.0:
            return super()._next_actions()
        _mlp_forward(_lib.load(), self._blob_ta, self.buffer._b_obs_, self._y4)
        td3_smooth_actions(self._y4, self._x_next, self.Do, self.k, sigma=self.target_noise, clip=self.noise_clip, seed=self.seed,
                           seq_base=self._noise_draws, central=self.central)
        self._noise_draws.add_(1)                                # fresh noise next update, and on every replay of a captured graph

    def _head(self, u, weight):
        c1, c2 = self.critics
        td3_head(c1.q, c2.q, c1.q_next, c2.q_next, self.buffer._b_rew, self.buffer._b_done, self.gamma, weight=weight,
                 out=(c1.g_q, c2.g_q, self._g_pi, self.td, self.stats[u]), workspace=self._head_ws)

    def _delayed(self, u):
        return (u + 1) % self.policy_delay == 0

    def _critics_step(self, u):
        super()._critics_step(u, polyak=self._delayed(u))

    def _actor_half(self, u):
        if self._delayed(u):
            super()._actor_half(u)
