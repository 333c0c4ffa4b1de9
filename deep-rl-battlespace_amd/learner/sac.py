"""The soft actor-critic update on device (csrc/bsx_sac_head.hip): what it adds to ddpg.py's and td3.py's calls, and the learner around it.

  sac_sample_actions, sac_head, sac_policy_seed, sac_policy_grad   the reparameterised draw with its log-probability into a critic input, the
                                                soft TD head of two critics, the actor's seeds through the smaller critic, the gradients
                                                of the actor's output, of log_std and of the temperature
  SACLearner(buffer, actor, critic=None, critic2=None, ...)   the Gaussian policy of PolicyRollout(sample="gaussian") trained from the ring; one graph

The learner is td3.py's _TwinCriticLearner -- DDPGLearner's sequence of steps over two critics -- with the steps that are SAC's own: the next
actions drawn from the current actor, the soft head, and an actor's half through both critics.  sac_head's argument check is ddpg.py's
_head_args, td_head's and td3_head's too.
"""
import math
from collections import namedtuple
from functools import partial

import torch

from .. import _lib
from .._args import _F32, _need, _number, _workspace
from ._common import _U64, _f32, _hyper, _int64_word, _ptr, _stream
from .adam import AdamState, adam_hyper, mlp_adam_step
from .ddpg import _batch_rows, _critic_width, _head_args, _head_rows
from .mlp import _mlp_forward, _mlp_grad
from .td3 import TD3_STATS, _TwinCriticLearner

SacHead = namedtuple("SacHead", "g_q1 g_q2 td stats")
SacPolicyGrad = namedtuple("SacPolicyGrad", "g_a4 g_log_std g_log_alpha stats")
SAC_STATS = TD3_STATS
SAC_PI_STATS = ("n", "actor_loss", "q_pi", "logp", "alpha", "weight", "picked_1", "reserved")
_FINITE = (lambda x: math.isfinite(x), "a finite number")
_F64 = (torch.float64,)


def _three(k):
    if int(k) != 3:
        raise ValueError(f"the Gaussian policy has three action columns: n_actions must be 3, got {k!r}")
    return 3


def sac_sample_actions(y4, log_std, x, obs_len, n_actions=3, *, seed=0, seq=0, seq_base=None, z=None, central=True, own_only=False,
                       out=None):
    """a ~ pi into the action columns of a critic input and log pi(a), in one launch (csrc/bsx_sac_head.hip, `bsx_sac_sample_actions`;
    include/battlespace_hip.h) -> (x, logp, z_out).

    y4 float32 [B, nA, 4]: the actor's output rows, mu in columns 0 .. 2; log_std float32 [nA, 3]; x float32 [B, nA, Dc].  Per (b, j) and
    column c, a = fmaf(expf(log_std[j, c]), z[c], mu[c]) and logp[b, j] = sum_c (-z_c^2 / 2 - log_std[j, c]) - 3 log(2 pi) / 2: the
    rollout's Gaussian head (PolicyRollout(sample="gaussian")), operation for operation, with no clamp and no tanh-squash correction.  a
    goes where ddpg_put_actions(own_only) writes; nothing else of x is written.  The noise is keyed by (b, j) alone.  z: float32
    [B, nA, 4], the normals (tests); without it they are the project's Philox normals under (seed, seq + seq_base, b nA + j) and a salt of
    their own (_lib.SAC_SALT).  seq_base: an int64 device word read on the device, or None.  out: (logp [B, nA], z_out [B, nA, 4] or
    None) to write into; without it both are new.  z_out receives the normals used, column 3 = +0.  n_actions must be 3."""
    Do, k = int(obs_len), _three(n_actions)
    B, nA, dev = _batch_rows(y4, "y4")
    Dc = _critic_width(nA, Do, k, central)
    need = partial(_need, dev=dev, anchor="y4")
    need(y4, "y4", (B, nA, 4), _F32)
    need(log_std, "log_std", (nA, 3), _F32)
    need(x, "x", (B, nA, Dc), _F32)
    if z is not None:
        need(z, "z", (B, nA, 4), _F32)
    if seq_base is not None:
        _int64_word(seq_base, "seq_base", dev, "y4")
    if out is None:
        out = (torch.empty((B, nA), dtype=torch.float32, device=dev), torch.empty((B, nA, 4), dtype=torch.float32, device=dev))
    logp, z_out = out
    need(logp, "out logp", (B, nA), _F32)
    if z_out is not None:
        need(z_out, "out z_out", (B, nA, 4), _F32)
    _lib.check(_lib.load().bsx_sac_sample_actions(y4.data_ptr(), log_std.data_ptr(), B, nA, Do, k, int(bool(central)), int(bool(own_only)),
                                                  int(seed) & _U64, int(seq) & _U64, _ptr(seq_base), _ptr(z), x.data_ptr(), logp.data_ptr(),
                                                  _ptr(z_out), _stream(dev)), "bsx_sac_sample_actions")
    return x, logp, z_out


def sac_head_workspace_bytes(B, nA):
    """Bytes of the workspace sac_head needs for B rows of nA agents."""
    return _lib.query_bytes("bsx_sac_head_workspace_bytes", B, nA)


def sac_head(q1, q2, q1_next, q2_next, logp_next, rew, done, log_alpha, gamma, *, weight=None, out=None, workspace=None):
    """The soft TD target of two target critics and both critics' grad_out, in one pass (csrc/bsx_sac_head.hip, `bsx_sac_head`; the exact
    contract is written out in include/battlespace_hip.h) -> SacHead(g_q1, g_q2, td, stats).

    q1, q2, q1_next, q2_next, logp_next, rew float32 [B, nA]; done uint8 or bool [B, nA]; log_alpha float32 [nA] on the device; weight
    float32 [B, nA] or None; gamma in [0, 1].  Per element m = min(q1_next, q2_next) (a NaN in either is a NaN), v = m - exp(log_alpha[i])
    logp_next, y = fmaf(gamma, done ? 0 : v, rew); g_q1, g_q2, td and stats (learner.SAC_STATS == TD3_STATS) are td3_head's expressions
    of y.  There is no g_pi (sac_policy_seed).  Deterministic; two launches on the current stream, no host synchronisation.  out: optional
    (g_q1, g_q2, td or None, stats) to write into and workspace (at least sac_head_workspace_bytes(B, nA) bytes, 8-byte aligned) -- pass
    both and nothing is allocated (a captured graph)."""
    rows = ((q1, "q1"), (q2, "q2"), (q1_next, "q1_next"), (q2_next, "q2_next"), (logp_next, "logp_next"), (rew, "rew"))
    B, nA, dev, gamma, (g_q1, g_q2, td, stats), workspace = _head_args("sac_head", rows, done, gamma, weight, ("g_q1", "g_q2"), out, workspace,
                                                                       per_agent=((log_alpha, "log_alpha"),))
    io = _lib.BsxSacIo(q1.data_ptr(), q2.data_ptr(), q1_next.data_ptr(), q2_next.data_ptr(), logp_next.data_ptr(), rew.data_ptr(), done.data_ptr(),
                       _ptr(weight), log_alpha.data_ptr(), g_q1.data_ptr(), g_q2.data_ptr(), _ptr(td))
    _lib.check(_lib.load().bsx_sac_head(_lib.ctypes.byref(io), B, nA, gamma, workspace.data_ptr(), stats.data_ptr(), _stream(dev)), "bsx_sac_head")
    return SacHead(g_q1, g_q2, td, stats)


def sac_policy_seed(q1_pi, q2_pi, *, weight=None, out=None):
    """The seeds of the two critics' input-gradient passes on x_pi, in one launch (`bsx_sac_policy_seed`) -> (g_pi1, g_pi2), float32
    [B, nA, 4].  q1_pi, q2_pi float32 [B, nA]: the critics on x_pi.  Per element critic 1 is picked where q1_pi < q2_pi or q1_pi is a NaN,
    else critic 2 (sac_head's rule for the smaller); the picked critic's seed is [..., 0] = -(w float(1 / B)), everything else +0: mlp_grad
    of each critic with its seed gives the input gradients of the sum over agents of -mean_b w min(Q1, Q2)(x_pi)."""
    B, nA, dev = _head_rows(q1_pi, "sac_policy_seed")
    need = partial(_need, dev=dev, anchor="q1_pi")
    need(q1_pi, "q1_pi", (B, nA), _F32)
    need(q2_pi, "q2_pi", (B, nA), _F32)
    if weight is not None:
        need(weight, "weight", (B, nA), _F32)
    if out is None:
        out = tuple(torch.empty((B, nA, 4), dtype=torch.float32, device=dev) for _ in range(2))
    g1, g2 = out
    need(g1, "out g_pi1", (B, nA, 4), _F32)
    need(g2, "out g_pi2", (B, nA, 4), _F32)
    _lib.check(_lib.load().bsx_sac_policy_seed(q1_pi.data_ptr(), q2_pi.data_ptr(), _ptr(weight), B, nA, g1.data_ptr(), g2.data_ptr(), _stream(dev)),
               "bsx_sac_policy_seed")
    return g1, g2


def sac_policy_grad_workspace_bytes(B, nA):
    """Bytes of the workspace sac_policy_grad needs for B rows of nA agents."""
    return _lib.query_bytes("bsx_sac_policy_grad_workspace_bytes", B, nA)


def sac_policy_grad(gx1, gx2, z, logp, q1_pi, q2_pi, log_std, log_alpha, obs_len, n_actions=3, *, target_entropy=-3.0, weight=None,
                    central=True, alpha_state=None, hyper=None, step=None, out=None, workspace=None):
    """The actor's grad_out, the gradients of log_std and of the log temperature, and the policy's statistics, in one pass and one merge
    (`bsx_sac_policy_grad`; include/battlespace_hip.h) -> SacPolicyGrad(g_a4, g_log_std, g_log_alpha, stats).

    gx1, gx2 float32 [B, nA, Dc]: the two critics' input gradients on x_pi (mlp_grad with sac_policy_seed's seeds); z [B, nA, 4] and logp
    [B, nA]: sac_sample_actions' outputs for the draw in x_pi; q1_pi, q2_pi [B, nA]; log_std [nA, 3]; log_alpha [nA].  g_a4 [B, nA, 4]: the
    own-action columns of gx1 + gx2, the actor's grad_out (squash=True).  g_log_std[i, c] = sum_b g_a4[b, i, c] exp(log_std[i, c]) z[b, i, c]
    - alpha_i sum_b w / B and g_log_alpha[i] = -sum_b (w / B) (logp[b, i] + target_entropy): float64 sums of float32 terms in a fixed
    order.  stats f64 [8] in the order of learner.SAC_PI_STATS.  alpha_state (an AdamState of log_alpha), hyper (adam_hyper's row) and
    step (an int64 device word): all three or none; given, log_alpha takes one Adam step in the same two launches (no clipping; the
    word advances by one), after it has been read for the gradients.  out: (g_a4, g_log_std, g_log_alpha, stats) and workspace (at
    least sac_policy_grad_workspace_bytes(B, nA) bytes): pass both and nothing is allocated."""
    Do, k = int(obs_len), _three(n_actions)
    B, nA, dev = _batch_rows(gx1, "gx1")
    Dc = _critic_width(nA, Do, k, central)
    te = _number(target_entropy, "target_entropy", *_FINITE)
    need = partial(_need, dev=dev, anchor="gx1")
    need(gx1, "gx1", (B, nA, Dc), _F32)
    need(gx2, "gx2", (B, nA, Dc), _F32)
    need(z, "z", (B, nA, 4), _F32)
    for x, name in ((logp, "logp"), (q1_pi, "q1_pi"), (q2_pi, "q2_pi")):
        need(x, name, (B, nA), _F32)
    if weight is not None:
        need(weight, "weight", (B, nA), _F32)
    need(log_std, "log_std", (nA, 3), _F32)
    need(log_alpha, "log_alpha", (nA,), _F32)
    given = [x is not None for x in (alpha_state, hyper, step)]
    if any(given) and not all(given):
        raise ValueError("alpha_state, hyper and step go together: all three or none")
    if all(given):
        if not isinstance(alpha_state, AdamState):
            raise TypeError("alpha_state must be an AdamState")
        need(alpha_state.m, "alpha_state.m", (nA,), _F32)
        need(alpha_state.v, "alpha_state.v", (nA,), _F32)
        need(hyper, "hyper", (8,), _F32)
        _int64_word(step, "step", dev, "gx1")
    if out is None:
        f = _f32(torch.empty, dev)
        out = (f(B, nA, 4), f(nA, 3), f(nA), torch.empty(8, dtype=torch.float64, device=dev))
    g_a4, g_ls, g_la, stats = out
    need(g_a4, "out g_a4", (B, nA, 4), _F32)
    need(g_ls, "out g_log_std", (nA, 3), _F32)
    need(g_la, "out g_log_alpha", (nA,), _F32)
    need(stats, "out stats", (8,), _F64)
    workspace = _workspace(workspace, sac_policy_grad_workspace_bytes(B, nA), dev)
    st = alpha_state
    io = _lib.BsxSacPolicyIo(gx1.data_ptr(), gx2.data_ptr(), z.data_ptr(), logp.data_ptr(), q1_pi.data_ptr(), q2_pi.data_ptr(), _ptr(weight),
                             log_std.data_ptr(), log_alpha.data_ptr(), g_a4.data_ptr(), g_ls.data_ptr(), g_la.data_ptr(),
                             _ptr(st.m if st else None), _ptr(st.v if st else None), _ptr(hyper), _ptr(step))
    _lib.check(_lib.load().bsx_sac_policy_grad(_lib.ctypes.byref(io), B, nA, Do, k, int(bool(central)), te, workspace.data_ptr(), stats.data_ptr(),
                                               _stream(dev)), "bsx_sac_policy_grad")
    return SacPolicyGrad(g_a4, g_ls, g_la, stats)


class SACLearner(_TwinCriticLearner):
    """The soft actor-critic update of a team from its replay ring, on device (Haarnoja et al. 2018, the twin-critic form with a learned
    temperature; per agent, with MADDPG's critic inputs): DDPGLearner's actor, ring and critic inputs, TD3Learner's two critics, and a
    stochastic policy -- the one PolicyRollout(sample="gaussian", log_std=...) plays: mu = the actor's tanh row, one learned log_std per
    agent and action column, a = mu + exp(log_std) z.  Its log-probability carries no tanh-squash correction (the clip to [-1, 1] belongs
    to the env), and the spread does not depend on the state: a state-dependent spread would need six head outputs and the fused MLP
    has four.  Both are out of scope here.

        log_std = torch.full((n, 3), math.log(0.2), device="cuda")
        ro = PolicyRollout(env, actor_all, T, sample="gaussian", log_std=log_std_all)
        learner = SACLearner(buf, actor, log_std=log_std)       # critics StackedActor(n, Dc, 1) are made, each with its own initialisation
        learner.capture()
        while training:
            ro.run(); buf.append_rollout(ro, range(n))
            stats = learner.update()                      # f64 [updates, 8] on the device, columns in the order of learner.SAC_STATS
            learner.publish(ro, range(n))                 # the actors and their spread

    Update u of a call, on the current stream, with cached buffers and no host synchronisation:
       1. buffer.sample(), ddpg_inputs
       2. the CURRENT actor on obs_next, sac_sample_actions(own_only=False) into x_next -> logp_next; keyed by `seed` and the device word
          `_noise_draws`, which then advances by 1
       3. both target critics on x_next, both critics on x_cur
       4. sac_head                                       y = r + gamma (1 - done) (min(q1_next, q2_next) - alpha logp_next), g_q1, g_q2, the statistics
          (a PrioritizedReplayBuffer: with weight = buffer.weights, then buffer.update_priorities(q1, y))
       5. mlp_grad of both critics, then ONE mlp_adam_step of both with both Polyak targets, every update
       6. the actor on obs, sac_sample_actions(own_only=True) into x_pi, logp and z kept; the word advances again
       7. both STEPPED critics on x_pi, sac_policy_seed
       8. mlp_grad of each critic on x_pi with its seed -> gx1, gx2
       9. sac_policy_grad -> g_a4, g_log_std, g_log_alpha, stats_pi; it steps log_alpha when lr_alpha is set
      10. mlp_grad of the actor, mlp_adam_step([actor], ..., log_std=...) without targets.

    buffer, actor, critic, critic2, critic_input, gamma, tau, the learning rates, betas, eps, max_grad_norm, updates: TD3Learner's; the
    buffer must have three action columns.  log_std: a contiguous float32 [nA, 3] tensor on the device, kept by reference and stepped in
    place with the actor (one clip norm over both) -- the rows of a rollout's log_std, or a tensor of the learner's own; one filled with
    log 0.2 is made if none is given.  alpha: the initial temperature of every agent (`log_alpha` float32 [nA]); lr_alpha: the rate of
    its Adam step (betas and eps as the networks', no clipping), None keeps log_alpha fixed and holds no Adam state; target_entropy: the
    entropy the temperature steers to, per agent, -3.0 by default (minus the action columns).  SAC has no target actor: the
    `target_actor` and `_blob_ta` the learner inherits from DDPGLearner are never read or stepped.  On top of DDPGLearner's state the
    learner owns `critic2`, `target_critic2`, their blobs, `adam_critic2`, `log_std`, `adam_log_std`, `log_alpha`, `adam_alpha`,
    `hyper_alpha`, `step_alpha` and `_noise_draws`; `stats` is f64 [updates, 8] in the order of SAC_STATS, `stats_pi` f64 [updates, 8] in
    the order of SAC_PI_STATS.  update(), capture() and sync() are DDPGLearner's over all of it; set_lr takes alpha= as well; publish also
    copies log_std into a rollout that has one.  Parameter sharing and a policy delay are not here.  On a ring filled through
    replay.NStepAppender the head's target is the n-step one when the learner is given gamma=app.bootstrap_gamma; it then carries the
    entropy term -alpha logp' at the bootstrap state only, not at the n - 1 states the folded reward passes."""

    def __init__(self, buffer, actor, critic=None, critic2=None, *, log_std=None, alpha=0.2, lr_alpha=3e-4, target_entropy=None,
                 critic_input="central", gamma=0.95, tau=0.01, lr_actor=1e-3, lr_critic=1e-3, betas=(0.9, 0.999), eps=1e-8,
                 max_grad_norm=None, updates=1, seed=0):
        alpha = _number(alpha, "alpha", lambda x: 0.0 < x < math.inf, "a finite number > 0")
        lr_alpha = None if lr_alpha is None else _hyper("lr", lr_alpha)
        self.target_entropy = _number(-3.0 if target_entropy is None else target_entropy, "target_entropy", *_FINITE)
        if getattr(buffer, "n_actions", 3) != 3:
            raise ValueError(f"SACLearner needs a buffer with 3 action columns (the Gaussian policy's), got {buffer.n_actions}")
        super().__init__(buffer, actor, critic, critic2, seed=seed, gx2=True, critic_input=critic_input, gamma=gamma, tau=tau, lr_actor=lr_actor,
                         lr_critic=lr_critic, betas=betas, eps=eps, max_grad_norm=max_grad_norm, updates=updates)
        nA, B, dev = self.nA, self.B, self._x_cur.device
        if log_std is None:
            log_std = torch.full((nA, 3), math.log(0.2), dtype=torch.float32, device=dev)
        _need(log_std, "log_std", (nA, 3), _F32, dev, "the buffer")
        self.log_std, self.adam_log_std = log_std, AdamState(log_std)
        self.log_alpha = torch.full((nA,), math.log(alpha), dtype=torch.float32, device=dev)
        self.learn_alpha = lr_alpha is not None
        self.adam_alpha = AdamState(self.log_alpha) if self.learn_alpha else None
        self.hyper_alpha = adam_hyper(lr_alpha, betas, eps, None, dev) if self.learn_alpha else None
        self.step_alpha = torch.zeros(1, dtype=torch.int64, device=dev)
        self.stats_pi = torch.zeros((self.updates, 8), dtype=torch.float64, device=dev)
        f = _f32(torch.zeros, dev)
        self._g_pi2, self._z = f(B, nA, 4), f(B, nA, 4)
        self._logp_next, self._logp, self._g_log_std, self._g_log_alpha = f(B, nA), f(B, nA), f(nA, 3), f(nA)
        self._pi_ws = _workspace(None, sac_policy_grad_workspace_bytes(B, nA), dev)

    def _next_actions(self):
        """Step 2: a draw from the CURRENT actor on obs_next into x_next, its log-probability kept; the sequence word advances."""
        _mlp_forward(_lib.load(), self._blob_a, self.buffer._b_obs_, self._y4)
        sac_sample_actions(self._y4, self.log_std, self._x_next, self.Do, self.k, seed=self.seed, seq_base=self._noise_draws,
                           central=self.central, own_only=False, out=(self._logp_next, None))
        self._noise_draws.add_(1)                                # fresh noise at the next draw, and on every replay of a captured graph

    def _head(self, u, weight):
        c1, c2 = self.critics
        sac_head(c1.q, c2.q, c1.q_next, c2.q_next, self._logp_next, self.buffer._b_rew, self.buffer._b_done, self.log_alpha, self.gamma,
                 weight=weight, out=(c1.g_q, c2.g_q, self.td, self.stats[u]), workspace=self._head_ws)

    def _actor_half(self, u):
        """Steps 6 to 10: the policy's, log_std's and the temperature's gradients through both stepped critics, and their steps."""
        lib, obs, (c1, c2) = _lib.load(), self.buffer._b_obs, self.critics
        Do, k, c = self.Do, self.k, self.central
        weight = self.buffer.weights if self._prioritized else None
        _mlp_forward(lib, self._blob_a, obs, self._y4)
        sac_sample_actions(self._y4, self.log_std, self._x_pi, Do, k, seed=self.seed, seq_base=self._noise_draws, central=c, own_only=True,
                           out=(self._logp, self._z))
        self._noise_draws.add_(1)
        for ci in (c1, c2):                                      # (q now holds the critic on x_pi)
            _mlp_forward(lib, ci.blob, self._x_pi, self._yq4, ci.q)
        sac_policy_seed(c1.q, c2.q, weight=weight, out=(self._g_pi, self._g_pi2))
        for ci, seed in ((c1, self._g_pi), (c2, self._g_pi2)):
            _mlp_grad(lib, ci.buf, ci.blob, self._x_pi, seed, False, ci.buf["gx"])
        sac_policy_grad(c1.buf["gx"], c2.buf["gx"], self._z, self._logp, c1.q, c2.q, self.log_std, self.log_alpha, Do, k,
                        target_entropy=self.target_entropy, weight=weight, central=c, alpha_state=self.adam_alpha, hyper=self.hyper_alpha,
                        step=self.step_alpha if self.learn_alpha else None,
                        out=(self._g_a4, self._g_log_std, self._g_log_alpha, self.stats_pi[u]), workspace=self._pi_ws)
        row_a = _mlp_grad(lib, self._buf_a, self._blob_a, obs, self._g_a4, True)
        mlp_adam_step([self.actor], [row_a], [self.adam_actor], [self._blob_a], self.hyper_actor, self.step_actor, log_std=self.log_std,
                      g_log_std=self._g_log_std, log_std_state=self.adam_log_std, stats=self.step_stats_actor[u], workspace=self._adam_ws)

    def _state(self):
        """Every tensor an update writes that outlives it."""
        alpha = [self.adam_alpha.m, self.adam_alpha.v] if self.learn_alpha else []
        return super()._state() + [self.stats_pi, self.log_std, self.adam_log_std.m, self.adam_log_std.v, self.log_alpha, self.step_alpha] + alpha

    def set_lr(self, actor=None, critic=None, alpha=None):
        """DDPGLearner.set_lr, and alpha=: the rate of the temperature's step (a learner made with lr_alpha=None has none to set)."""
        super().set_lr(actor, critic)
        if alpha is not None:
            if not self.learn_alpha:
                raise ValueError("this learner keeps log_alpha fixed (lr_alpha=None): there is no rate to set")
            self.hyper_alpha[0].fill_(_hyper("lr", alpha))

    def publish(self, rollout, columns):
        """DDPGLearner.publish; a rollout with a `log_std` (sample="gaussian") also receives the learner's into its rows c0 : c0 + nA -- a
        device copy on the current stream (a no-op in effect when the learner was given those rows themselves)."""
        super().publish(rollout, columns)
        ls = getattr(rollout, "log_std", None)
        if ls is not None:
            c0 = int(list(columns)[0])
            dst = ls[c0:c0 + self.nA]
            if dst.data_ptr() != self.log_std.data_ptr():
                with torch.no_grad():
                    dst.copy_(self.log_std)
