"""The TD3 / MATD3 update on device (csrc/bsx_td3_head.hip): what it adds to ddpg.py's calls, and the learner around it.

  td3_smooth_actions, td3_head                  target policy smoothing into x_next, the TD head of two critics
  TD3Learner(buffer, actor, critic=None, critic2=None, ...)   twin critics, smoothed targets, a delayed actor and target step; one graph
"""
import copy
from collections import namedtuple
from functools import partial

import torch

from .. import _lib
from .._args import _F32, _FLAG, _need, _workspace
from ..rollout import StackedActor
from ._common import _WEIGHT, _f32, _hyper, _int64_word, _stream
from .adam import AdamState, mlp_adam_step, mlp_adam_step_workspace_bytes
from .ddpg import DDPGLearner, _batch_rows, _critic_width, ddpg_action_grad, ddpg_inputs, ddpg_put_actions
from .mlp import PARAMS, _buffers, _check_mlp, _mlp_forward, _mlp_grad

Td3Head = namedtuple("Td3Head", "g_q1 g_q2 g_pi td stats")
TD3_STATS = ("n", "critic_loss", "q", "target", "abs_td", "done", "weight", "q_gap")
_U64 = (1 << 64) - 1


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
                                                  seq_base.data_ptr() if seq_base is not None else None,
                                                  z.data_ptr() if z is not None else None, x.data_ptr(), _stream(dev)), "bsx_td3_smooth_actions")
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
    if not isinstance(q1, torch.Tensor) or q1.dim() != 2:
        raise ValueError("q1 must be a float32 [B, nA] tensor")
    dev, (B, nA) = q1.device, q1.shape
    if dev.type != "cuda":
        raise ValueError("td3_head runs on the GPU: q1 is on " + str(dev))
    if not 1 <= B < 1 << 31 or not 1 <= nA <= _lib.MAX_N:
        raise ValueError(f"q1 has shape {tuple(q1.shape)}: 1 <= B < 2^31 and 1 .. {_lib.MAX_N} agents are needed")
    gamma = _hyper("gamma", gamma)
    need = partial(_need, dev=dev, anchor="q1")
    for x, name in ((q1, "q1"), (q2, "q2"), (q1_next, "q1_next"), (q2_next, "q2_next"), (rew, "rew")):
        need(x, name, (B, nA), _F32)
    need(done, "done", (B, nA), _FLAG)
    if weight is not None:
        need(weight, "weight", (B, nA), _F32)
    if out is None:
        f = _f32(torch.empty, dev)
        out = (f(B, nA, 4), f(B, nA, 4), f(B, nA, 4), f(B, nA), torch.empty(8, dtype=torch.float64, device=dev))
    g_q1, g_q2, g_pi, td, stats = out
    for x, name in ((g_q1, "out g_q1"), (g_q2, "out g_q2"), (g_pi, "out g_pi")):
        need(x, name, (B, nA, 4), _F32)
    if td is not None:
        need(td, "out td", (B, nA), _F32)
    need(stats, "out stats", (8,), (torch.float64,))
    workspace = _workspace(workspace, td3_head_workspace_bytes(B, nA), dev)
    io = _lib.BsxTd3Io(q1.data_ptr(), q2.data_ptr(), q1_next.data_ptr(), q2_next.data_ptr(), rew.data_ptr(), done.data_ptr(),
                       weight.data_ptr() if weight is not None else None, g_q1.data_ptr(), g_q2.data_ptr(), g_pi.data_ptr(),
                       td.data_ptr() if td is not None else None)
    _lib.check(_lib.load().bsx_td3_head(_lib.ctypes.byref(io), B, nA, gamma, workspace.data_ptr(), stats.data_ptr(), _stream(dev)), "bsx_td3_head")
    return Td3Head(g_q1, g_q2, g_pi, td, stats)


class TD3Learner(DDPGLearner):
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
    actor step stay as they were.  update(), capture(), set_lr(), sync() (six blobs) and publish() are DDPGLearner's.  Parameter
    sharing is not here.  On a ring filled through replay.NStepAppender the head's target is the n-step one when the learner is given
    gamma=app.bootstrap_gamma."""

    def __init__(self, buffer, actor, critic=None, critic2=None, *, critic_input="central", gamma=0.95, tau=0.01, lr_actor=1e-3,
                 lr_critic=1e-3, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=None, updates=2, policy_delay=2, target_noise=0.2,
                 noise_clip=0.5, seed=0):
        if critic2 is not None and critic2 is critic:
            raise ValueError("critic2 is critic itself: the second critic is a network of its own")
        if isinstance(policy_delay, bool) or not isinstance(policy_delay, int) or policy_delay < 1:
            raise ValueError(f"policy_delay must be an int >= 1, got {policy_delay!r}")
        if int(updates) < 1 or int(updates) % policy_delay:
            raise ValueError(f"updates must be a multiple of policy_delay = {policy_delay} (a call keeps the schedule), got {updates!r}")
        self.policy_delay = policy_delay
        self.target_noise, self.noise_clip = _hyper("target_noise", target_noise, _WEIGHT), _hyper("noise_clip", noise_clip, _WEIGHT)
        self.seed = int(seed)
        super().__init__(buffer, actor, critic, critic_input=critic_input, gamma=gamma, tau=tau, lr_actor=lr_actor, lr_critic=lr_critic,
                         betas=betas, eps=eps, max_grad_norm=max_grad_norm, updates=updates)
        nA, B, Dc, dev = self.nA, self.B, self.Dc, self._x_cur.device
        if critic2 is None:
            critic2 = StackedActor(nA, Dc, 1, device=dev)
        have = tuple(getattr(critic2, a, None) for a in ("n_actors", "obs_len", "n_actions"))
        if have != (nA, Dc, 1):
            raise ValueError(f"critic2 must be a StackedActor{(nA, Dc, 1)} for this buffer and critic_input={critic_input!r}, got "
                             f"{'StackedActor' + str(have) if None not in have else type(critic2).__name__}")
        _check_mlp(critic2, self._x_cur, False, "TD3Learner")
        self.critic2, self.target_critic2 = critic2, copy.deepcopy(critic2)
        self.target_critic2.__dict__.pop("_bsx_mlp_buffers", None)
        self.target_critic2.requires_grad_(False)
        self._blob_c2, self._blob_tc2 = critic2.pack(), self.target_critic2.pack()
        self.adam_critic2 = AdamState(critic2)
        f = _f32(torch.zeros, dev)
        self._g_q2, self._q2, self._q2_next = f(B, nA, 4), f(B, nA), f(B, nA)
        self._noise_draws = torch.zeros(1, dtype=torch.int64, device=dev)       # the smoothing's sequence word, advanced once per smoothed update
        self._head_ws = _workspace(None, td3_head_workspace_bytes(B, nA), dev)
        self._adam_ws = _workspace(None, max(mlp_adam_step_workspace_bytes(nA, 1), mlp_adam_step_workspace_bytes(nA, 2)), dev)
        self._buf_c2 = _buffers(critic2).get(B, nA, Dc, dev)

    def _update(self, u):
        """Update u of a call: the six steps of the class's docstring."""
        lib, buf = _lib.load(), self.buffer
        buf.sample()
        obs, obs_next, act, rew, done = buf._b_obs, buf._b_obs_, buf._b_act, buf._b_rew, buf._b_done
        Do, k, c = self.Do, self.k, self.central
        ddpg_inputs(obs, obs_next, act, central=c, out=(self._x_cur, self._x_next, self._x_pi))
        _mlp_forward(lib, self._blob_ta, obs_next, self._y4)
        if self.target_noise > 0.0:
            td3_smooth_actions(self._y4, self._x_next, Do, k, sigma=self.target_noise, clip=self.noise_clip, seed=self.seed,
                               seq_base=self._noise_draws, central=c)
            self._noise_draws.add_(1)                            # fresh noise next update, and on every replay of a captured graph
        else:
            ddpg_put_actions(self._y4, self._x_next, Do, k, central=c, own_only=False)
        _mlp_forward(lib, self._blob_tc, self._x_next, self._yq4, self._q_next)
        _mlp_forward(lib, self._blob_tc2, self._x_next, self._yq4, self._q2_next)
        _mlp_forward(lib, self._blob_c, self._x_cur, self._yq4, self._q)
        _mlp_forward(lib, self._blob_c2, self._x_cur, self._yq4, self._q2)
        td3_head(self._q, self._q2, self._q_next, self._q2_next, rew, done, self.gamma, weight=buf.weights if self._prioritized else None,
                 out=(self._g_q, self._g_q2, self._g_pi, self.td, self.stats[u]), workspace=self._head_ws)
        if self._prioritized:
            buf.update_priorities(self._q, self.td)
        row_c = _mlp_grad(lib, self._buf_c, self._blob_c, self._x_cur, self._g_q, False)
        row_c2 = _mlp_grad(lib, self._buf_c2, self._blob_c2, self._x_cur, self._g_q2, False)
        delayed = (u + 1) % self.policy_delay == 0
        both = dict(targets=[self.target_critic, self.target_critic2], target_blobs=[self._blob_tc, self._blob_tc2]) if delayed else {}
        mlp_adam_step([self.critic, self.critic2], [row_c, row_c2], [self.adam_critic, self.adam_critic2], [self._blob_c, self._blob_c2],
                      self.hyper_critic, self.step_critic, stats=self.step_stats_critic[u], workspace=self._adam_ws, **both)
        if not delayed:
            return
        _mlp_forward(lib, self._blob_a, obs, self._y4)
        ddpg_put_actions(self._y4, self._x_pi, Do, k, central=c, own_only=True)
        _mlp_grad(lib, self._buf_c, self._blob_c, self._x_pi, self._g_pi, False, self._buf_c["gx"])
        ddpg_action_grad(self._buf_c["gx"], Do, k, central=c, out=self._g_a4)
        row_a = _mlp_grad(lib, self._buf_a, self._blob_a, obs, self._g_a4, True)
        mlp_adam_step([self.actor], [row_a], [self.adam_actor], [self._blob_a], self.hyper_actor, self.step_actor,
                      targets=[self.target_actor], target_blobs=[self._blob_ta], stats=self.step_stats_actor[u], workspace=self._adam_ws)

    def _state(self):
        """Every tensor an update writes that outlives it."""
        return (super()._state() + [self._noise_draws, self._blob_c2, self._blob_tc2, self.adam_critic2.m, self.adam_critic2.v]
                + [getattr(net, p) for net in (self.critic2, self.target_critic2) for p in PARAMS])

    def sync(self):
        """Re-pack all six blobs from their networks, once: for a caller who has edited parameters or targets from outside."""
        super().sync()
        self.critic2.pack(out=self._blob_c2)
        self.target_critic2.pack(out=self._blob_tc2)
