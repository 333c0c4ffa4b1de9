"""The PPO update on device (csrc/bsx_ppo_head.hip): the loss head between the fused forward and backward, and the learner around it.

  ppo_head(kind, y, v, rec, logp_old, adv, ret, mask, ...)      from the forward's outputs and a rollout's records to both grad_out tensors, one pass
  joint_width(n, Do), joint_obs(obs)                            a centralised critic's input width and rows: own observation first, then the team-mates'
  PPOLearner(rollout, ...)                                      the PPO update of a PolicyRollout's networks; device_step=True, capture(): one graph;
                                                                on a PolicyRollout(central_critic=) it is MAPPO's: a critic on the team's joint observation
"""
from collections import namedtuple
from functools import partial

import torch

from .. import _lib
from .._args import _F32, _FLAG, _need, _workspace
from ._common import _POSITIVE, _capture, _f32, _hyper, _stream
from .adam import (AdamState, adam_hyper, adam_step, adam_step_workspace_bytes, is_tied, mlp_adam_step, mlp_adam_step_workspace_bytes, share_group,
                   tie_)
from .mlp import PARAMS, _actor_forward, _buffers, _check_mlp, _mlp_forward, _mlp_grad, split_grad
from .shuffle import Minibatch, _word, minibatch_gather

PpoHead = namedtuple("PpoHead", "g_pi g_v g_log_std stats")
KINDS = {"categorical": 0, "gaussian": 1, 0: 0, 1: 1}
STATS = ("n", "loss", "policy_loss", "value_loss", "entropy", "approx_kl", "clip_fraction", "reserved")


def ppo_head_workspace_bytes(R, A):
    """Bytes of the workspace ppo_head needs for R rows of A agents."""
    return _lib.query_bytes("bsx_ppo_head_workspace_bytes", R, A)


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
    for x, name, tail in ((y, "y", (A, 4)), (v, "v", (A,)), (rec, "rec", (A, 4)), (logp_old, "logp_old", (A,)), (adv, "adv", (A,)), (ret, "ret", (A,))):
        need(x, name, (*lead, *tail), _F32)
    need(mask, "mask", (*lead, A), _FLAG)
    clip, c_v, c_e, temperature = _hyper("clip", clip), _hyper("c_v", c_v), _hyper("c_e", c_e), _hyper("temperature", temperature)
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
        f = _f32(torch.empty, dev)
        out = (f(*lead, A, 4), f(*lead, A, 4), f(A, 3) if k == 1 else None, torch.empty(8, dtype=torch.float64, device=dev))
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
                                        workspace.data_ptr(), stats.data_ptr(), _stream(dev)), "bsx_ppo_head")
    return PpoHead(g_pi, g_v, g_ls if k == 1 else None, stats)


JOINT_MAX_N = 4


def joint_width(n, Do=None):
    """n * Do: the inputs of a centralised critic of a team of n planes (1 .. 4) whose observations have Do floats (None: the env's
    3n + 2) -- 5, 16, 33 and 56 for 1v1 ... 4v4.  ValueError for another n, or a width the fused MLP kernels do not take (5v5: 85)."""
    n = int(n)
    Do = 3 * n + 2 if Do is None else int(Do)
    if not 1 <= n <= JOINT_MAX_N or Do < 1:
        raise ValueError(f"a central critic joins the observations of a team of 1 .. {JOINT_MAX_N} planes, each of at least one float: got "
                         f"n = {n} and Do = {Do} ({n} x {Do} = {n * Do} inputs; the fused MLP kernels take at most {_lib.MLP_MAX_D})")
    if n * Do > _lib.MLP_MAX_D:
        raise ValueError(f"a central critic of a team of {n} planes reads {n} x {Do} = {n * Do} inputs: the fused MLP kernels take at most "
                         f"{_lib.MLP_MAX_D}")
    return n * Do


def joint_obs(obs, *, out=None):
    """The input rows of a centralised critic from observation records, in one launch (csrc/bsx_ppo_central.hip, `bsx_ppo_joint_obs`;
    the contract is written out in include/battlespace_hip.h) -> x float32 [..., A, n Do].  obs float32 [..., A, Do], contiguous, on the
    GPU, A = 2n planes in two teams of n adjacent columns, 1 <= n <= 4 and n Do <= 64; leading axes are flattened.  Row (.., i) of x is
    plane i's own observation followed by its team-mates' in ascending plane index, as bit copies; nothing is masked.  out: the tensor
    to write into (nothing is allocated then: a captured graph)."""
    if not isinstance(obs, torch.Tensor) or obs.dim() < 2:
        raise ValueError("obs must be a float32 [..., A, Do] tensor")
    if obs.device.type != "cuda":
        raise ValueError(f"joint_obs runs on the GPU: obs is on {obs.device}")
    dev, (A, Do) = obs.device, obs.shape[-2:]
    if A < 2 or A % 2:
        raise ValueError(f"obs has shape {tuple(obs.shape)}: an even number of planes A = 2n is needed")
    width = joint_width(A // 2, Do)
    lead = tuple(obs.shape[:-2])
    need = partial(_need, dev=dev, anchor="obs")
    need(obs, "obs", (*lead, A, Do), _F32)
    if out is None:
        out = torch.empty((*lead, A, width), dtype=torch.float32, device=dev)
    need(out, "out", (*lead, A, width), _F32)
    if obs.numel():
        _lib.check(_lib.load().bsx_ppo_joint_obs(obs.data_ptr(), obs.numel() // (A * Do), A, Do, out.data_ptr(), _stream(dev)), "bsx_ppo_joint_obs")
    return out


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

    A centralised critic (MAPPO): on a PolicyRollout(central_critic=net) `critic` is that net, a StackedActor(A, joint_width(n), 1), and
    `critic_input` is "central" ("own" otherwise).  A minibatch is then six calls: the actor's forward WITHOUT a value head, joint_obs of
    the minibatch's observation rows into a cached [R, A, n D] buffer, bsx_mlp_forward of the critic on it (its raw column is v),
    ppo_head, bsx_mlp_grad of the actor on obs and of the critic on the joined rows.  The two networks no longer share a shape and are
    stepped one after the other, each clipped by its OWN gradient norm: device_step=True is adam_step of the actor (and log_std) into
    step_count / step_stats, then mlp_adam_step of the critic into critic_step_count / critic_step_stats, both with group=; they read
    ONE `hyper` tensor unless lr_critic= gives the critic a second one (`hyper_critic`; set_lr(lr, critic=)).  device_step=False clips
    the actor's parameters (with log_std) and the critic's separately and steps one torch optimiser (lr_critic: a parameter group).
    vclip, both kinds, shuffle=True, share= (is_tied is asked of the central critic too) and a scripted opponent are as above.

    rollout: a PolicyRollout with sample="categorical" or "gaussian", a value_actor or a central_critic, and gae= (ValueError otherwise).  vclip: clip the
    value loss around the rollout's recorded values.  optimizer: any torch optimiser over the parameters, instead of Adam(lr, betas, eps)
    (a ValueError with device_step=True)."""

    def __init__(self, rollout, *, clip=0.2, c_v=0.5, c_e=0.01, vclip=None, epochs=4, minibatches=4, lr=3e-4, max_grad_norm=None, optimizer=None,
                 device_step=False, betas=(0.9, 0.999), eps=1e-8, shuffle=False, shuffle_seed=None, share=None, lr_critic=None):
        ro = rollout
        if getattr(ro, "_sample", None) is None and getattr(ro, "_gauss", None) is None:
            raise ValueError("PPOLearner needs a PolicyRollout with sample='categorical' or 'gaussian' (it reads the recorded logp)")
        self.central = getattr(ro, "_central_w", None) is not None
        if (getattr(ro, "_value_w", None) is None and not self.central) or getattr(ro, "_gae", None) is None:
            raise ValueError("PPOLearner needs a PolicyRollout with a value_actor or a central_critic, and gae= (it reads value, adv, ret and mask)")
        epochs, minibatches = int(epochs), int(minibatches)
        if epochs < 1 or minibatches < 1 or ro.T % minibatches:
            raise ValueError(f"epochs >= 1 and a minibatches >= 1 that divides T = {ro.T} are needed (a minibatch is a range of whole ticks)")
        if not isinstance(shuffle, bool):
            raise ValueError(f"shuffle must be True or False, got {shuffle!r}")
        if shuffle_seed is not None and not shuffle:
            raise ValueError("shuffle_seed belongs to shuffle=True")
        self.shuffle = shuffle
        self.shuffle_seed = (int(ro.fused.seed) & ((1 << 64) - 1) if shuffle_seed is None else _word(shuffle_seed, "shuffle_seed")) if shuffle else None
        self.rollout, self.actor, self.critic = ro, ro.actor, ro.central_critic if self.central else ro.value_actor
        self.critic_input = "central" if self.central else "own"
        self._ro_blob_v = ro._central_w if self.central else ro._value_w                # the critic's blob the rollout reads
        if lr_critic is not None and (not self.central or optimizer is not None):
            raise ValueError("lr_critic is for a central critic, which is stepped on its own (and not with an optimizer= of the caller's)")
        self.kind = "gaussian" if ro._gauss is not None else "categorical"
        self.temperature = ro._sample["temperature"] if self.kind == "categorical" else 1.0
        self.log_std = ro.log_std if self.kind == "gaussian" else None
        self.clip, self.c_v, self.c_e = _hyper("clip", clip), _hyper("c_v", c_v), _hyper("c_e", c_e)
        self.vclip = None if vclip is None else _hyper("vclip", vclip)
        self.epochs, self.minibatches = epochs, minibatches
        self.max_grad_norm = None if max_grad_norm is None else _hyper("max_grad_norm", max_grad_norm, _POSITIVE)   # (no clipping is None here)
        _check_mlp(self.actor, ro.obs[:1], True, "fused_apply", obs_shaped=True)     # the observation check, under fused_apply's name
        A = self.actor.n_actors
        if self.central:
            _check_mlp(self.critic, ro._central_x[:1], False, "fused_mlp")
        else:
            _check_mlp(self.critic, ro.obs[:1], True, "fused_apply", obs_shaped=True)
        self.group = share_group(share, A // 2)
        if self.group > 1:
            if getattr(ro, "opponent", None) is not None and self.group == A:
                raise ValueError("a rollout with a scripted opponent cannot share one policy across both teams (share='all'): the scripted "
                                 "team's parameters are left alone; use share='team'")
            critic_name, critic_blob = ("central_critic", "ro._central_w") if self.central else ("value_actor", "ro._value_w")
            for name, x in (("actor", self.actor), (critic_name, self.critic), ("log_std", self.log_std)):
                if x is not None and not is_tied(x, self.group):
                    raise ValueError(f"share={share!r} needs networks that are already shared: the rollout's {name} differs inside a group of "
                                     f"{self.group} agents.  Tie actor, {critic_name} and log_std with learner.tie_(x, {self.group}) before "
                                     "building the PolicyRollout, or tie them and re-pack with ro.fused.refresh() and "
                                     f"critic.pack(out={critic_blob})")
        self._params_a = [getattr(self.actor, k) for k in PARAMS] + ([self.log_std] if self.log_std is not None else [])
        self._params_v = [getattr(self.critic, k) for k in PARAMS]
        self.params = self._params_a[:len(PARAMS)] + self._params_v + self._params_a[len(PARAMS):]
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
            self._adam_ws = _workspace(None, adam_step_workspace_bytes(A // 2, 1 if self.central else 2), dev)
            self._blob_a, self._blob_v = ro.fused.weights, self._ro_blob_v   # the step packs into the blobs the rollout plays from
            if self.central:                 # the critic is stepped on its own (mlp_adam_step: its width is not the actor's), with its own norm
                self.hyper_critic = self.hyper if lr_critic is None else adam_hyper(lr_critic, betas, eps, self.max_grad_norm, dev)
                self.critic_step_count = torch.zeros(1, dtype=torch.int64, device=dev)
                self.critic_step_stats = torch.zeros((epochs * minibatches, 4), dtype=torch.float64, device=dev)
                self._adam_ws_v = _workspace(None, mlp_adam_step_workspace_bytes(A, 1), dev)
        else:
            if optimizer is None:
                groups = self.params if lr_critic is None else [dict(params=self._params_a), dict(params=self._params_v, lr=_hyper("lr", lr_critic))]
                optimizer = torch.optim.Adam(groups, lr=lr, betas=betas, eps=eps)
            self.optimizer = optimizer
            self._blob_a, self._blob_v = torch.empty_like(ro.fused.weights), torch.empty_like(self._ro_blob_v)
        self._by_rows = {}
        self.stats = torch.zeros((epochs * minibatches, 8), dtype=torch.float64, device=dev)
        if shuffle:
            T, E, A, D = ro.T, *ro.obs.shape[1:]
            R = T * E // minibatches
            f = _f32(torch.empty, dev)
            self.shuffle_base = torch.zeros(1, dtype=torch.int64, device=dev)
            self.minibatch_idx = torch.zeros((epochs * minibatches, R), dtype=torch.int64, device=dev)
            self._gathered = Minibatch(f(R, A, D), f(R, A, 4), f(R, A), f(R, A), f(R, A), torch.empty((R, A), dtype=torch.uint8, device=dev),
                                       f(R, A) if self.vclip is not None else None)

    def _head_buffers(self, R):
        """The forward's outputs and the head's, per row count: allocated once."""
        if R not in self._by_rows:
            A, dev = self.actor.n_actors, self.rollout.obs.device
            f = _f32(torch.empty, dev)
            self._by_rows[R] = dict(y=f(R, A, 4), v=f(R, A), g_pi=f(R, A, 4), g_v=f(R, A, 4),
                                    x=f(R, A, self.critic.obs_len) if self.central else None, y_v=f(R, A, 4) if self.central else None,
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
        """The five calls of a minibatch on its records `mb` (a Minibatch of R contiguous rows: views of a tick range, or gathered); six
        with a central critic, whose forward is a call of its own on the join of the same rows."""
        lib, obs = _lib.load(), mb.obs
        (R, A, D), dev = obs.shape, obs.device
        b = self._head_buffers(R)
        if pack:
            self.actor.pack(out=self._blob_a)
            self.critic.pack(out=self._blob_v)
        if self.central:             # the actor without a value head; the critic on the join of the same rows, its raw column the value
            _actor_forward(lib, self._blob_a, obs, b["y"])
            x = joint_obs(obs, out=b["x"])
            _mlp_forward(lib, self._blob_v, x, b["y_v"], raw=b["v"])
        else:
            x = obs
            _actor_forward(lib, self._blob_a, obs, b["y"], self._blob_v, b["v"])
        head = ppo_head(self.kind, b["y"], b["v"], mb.rec, mb.logp, mb.adv, mb.ret, mb.mask,
                        clip=self.clip, c_v=self.c_v, c_e=self.c_e, temperature=self.temperature, log_std=self.log_std,
                        v_old=mb.value, vclip=self.vclip,
                        out=(b["g_pi"], b["g_v"], b["g_ls"], b["stats"] if stats is None else stats), workspace=b["ws"])
        # the head's outputs ARE bsx_mlp_grad's grad_out (four columns, the unused ones +0): mlp_grad's call without its padded copy
        row_a = _mlp_grad(lib, _buffers(self.actor).get(R, A, D, dev), self._blob_a, obs, head.g_pi, True)
        row_v = _mlp_grad(lib, _buffers(self.critic).get(R, A, x.shape[2], dev), self._blob_v, x, head.g_v, False)
        return row_a, row_v, head.g_log_std, head.stats

    def install(self, row_a, row_v, g_log_std):
        """The gradient rows onto the parameters' .grad (copies: the rows are overwritten by the next minibatch).  With share=: every
        group's sum (float32, in agent order from the leader's row on) on its leader's slice and +0 on its followers'."""
        with torch.no_grad():
            todo = [(getattr(net, k), g) for net, row in ((self.actor, row_a), (self.critic, row_v))
                    for k, g in zip(PARAMS, split_grad(self._group_sum(row), net.n_actions))]
            if self.log_std is not None:
                todo.append((self.log_std, self._group_sum(g_log_std)))
            for p, g in todo:
                if p.grad is None:
                    p.grad = torch.empty_like(p)
                p.grad.copy_(g)

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

    def _step_grads(self, i, **kw):
        """The gradients of optimiser step i of an update: its shuffled rows, or the whole ticks of minibatch i % minibatches (the
        minibatches in tick order in every epoch)."""
        if self.shuffle:
            return self.shuffled_grads(i, **kw)
        span, m = self.rollout.T // self.minibatches, i % self.minibatches
        return self.minibatch_grads(m * span, (m + 1) * span, **kw)

    def update(self):
        """epochs x minibatches optimiser steps over the rollout's current records, the minibatches in tick order in every epoch (shuffle=True:
        a fresh permutation of the rows per epoch); then the rollout's packed weights are refreshed.  -> stats f64 [epochs * minibatches, 8] on the device (a cached buffer; no host sync)."""
        ro = self.rollout
        if self.device_step:
            (self._graph.replay if self._graph is not None else self._device_update)()
            return self.stats
        for i in range(self.epochs * self.minibatches):
            row_a, row_v, g_ls, stats = self._step_grads(i)
            self.install(row_a, row_v, g_ls)
            if self.max_grad_norm is not None:
                if self.central:                       # each network's own norm, as MAPPO clips them
                    torch.nn.utils.clip_grad_norm_(self._params_a, self.max_grad_norm)
                    torch.nn.utils.clip_grad_norm_(self._params_v, self.max_grad_norm)
                else:
                    torch.nn.utils.clip_grad_norm_(self.params, self.max_grad_norm)
            self.optimizer.step()
            self._tie_params()
            self.stats[i].copy_(stats)
        ro.fused.refresh()
        self.critic.pack(out=self._ro_blob_v)
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
        for i in range(self.epochs * self.minibatches):
            row_a, row_v, g_ls, _ = self._step_grads(i, pack=False, stats=self.stats[i])
            both = not self.central
            adam_step([self.actor, self.critic] if both else [self.actor], [row_a, row_v] if both else [row_a],
                      [self.adam_a, self.adam_v] if both else [self.adam_a], [self._blob_a, self._blob_v] if both else [self._blob_a], self.hyper,
                      self.step_count, log_std=ls, g_log_std=g_ls if ls is not None else None, log_std_state=self.adam_ls,
                      stats=self.step_stats[i], workspace=self._adam_ws, group=self.group)
            if self.central:
                mlp_adam_step([self.critic], [row_v], [self.adam_v], [self._blob_v], self.hyper_critic, self.critic_step_count,
                              stats=self.critic_step_stats[i], workspace=self._adam_ws_v, group=self.group)
        if self.shuffle:
            self.shuffle_base.add_(self.epochs)                  # on the stream, inside a captured update: the next one draws afresh

    def _state(self):
        """Every tensor an update writes that outlives it."""
        return (list(self.params) + [self.adam_a.m, self.adam_a.v, self.adam_v.m, self.adam_v.v, self.step_count, self._blob_a, self._blob_v,
                                     self.stats, self.step_stats] + ([self.adam_ls.m, self.adam_ls.v] if self.adam_ls is not None else [])
                + ([self.shuffle_base, self.minibatch_idx] if self.shuffle else [])
                + ([self.critic_step_count, self.critic_step_stats] if self.central else []))

    def set_lr(self, lr, critic=None):
        """The learning rate of the steps from now on, written to `hyper` on the device (a fill on the current stream: no host
        synchronisation); a captured update reads it at every replay.  A central critic reads the same tensor, so it follows; built
        with lr_critic= it has a `hyper_critic` of its own, which critic= sets."""
        self._need_device_step("set_lr")
        if critic is not None and (not self.central or self.hyper_critic is self.hyper):
            raise ValueError("set_lr(critic=) needs a central critic built with lr_critic= (one rate tensor is shared otherwise)")
        self.hyper[0].fill_(_hyper("lr", lr))
        if critic is not None:
            self.hyper_critic[0].fill_(_hyper("lr", critic))

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
        self._graph = _capture(self._device_update, self._state, self.rollout.obs.device)
        return self
