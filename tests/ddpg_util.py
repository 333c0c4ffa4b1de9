"""What the tests of the DDPG head kernels (csrc/bsx_ddpg_head.hip: learner.ddpg_inputs, ddpg_put_actions, td_head, ddpg_action_grad)
and of DDPGLearner share, on top of tests/offpolicy_util.py (the head's machinery, the reference step, the kink filter, Hand, the bandit):

  SHAPES / plan      (B, nA, Do, k, central) at the smallest sizes each mechanism can go wrong at; the head's launch plan restated
  join, ref_inputs, ref_put_actions, ref_action_grad   the three copies' contracts of include/battlespace_hip.h restated in numpy, on
                     arrays of any dtype (they move bits)
  td_inputs / HEAD   the TD head's inputs (rounded to float32 once) and its kind: the target from q_next, g_q and g_pi.  offpolicy_util.Head
                     writes the rest over that: the float64 contract, the head as a torch user writes it with autograd from q -- in
                     float64 the check of the restatement, in float32 the yardstick --, both cached per shape, and yardstick_util's
                     bounds: (2 x mean, 4 x max) of the yardstick's error for g_q, g_pi and td (a wider factor only where
                     profiles/ddpg_float64.json records one and why), stats within its scalar_bound of own_error, the yardstick's own
                     error over 9 row orders
  learner_case       networks (mlp_grad_util.make_net "gains", w3 scaled by 60 and 100 as mlp_grad_util.ddpg_case does), ring rows, a
                     fixed batch and the row weights that leave every ReLU kink out, chosen in float64 alone
  joined / joined_pi the critic's inputs as a torch user writes them: the one torch statement of the join every composition here reads
  maddpg_grads       the critic's and the actor's gradients of the two MADDPG losses by torch autograd on the CPU, in any dtype
  stepped_case / update_reference   a whole update from target networks that are NOT the networks: the critic's gradient, the critic's
                     step with its Polyak target (adam_mlp_util.reference_step), the actor's gradient at the STEPPED critic, the actor's
                     step, the statistics -- in float64, and the same in float32 on the CPU as the yardstick; the row weights leave
                     the stepped critic's kinks out too (a fixed point); wrong_variants: the misreadings the case tells apart;
                     stepped_spread / stepped_exceptions / stepped_factor_of: the yardstick's own spread over row orders and the factors
                     profiles/ddpg_float64.json records from it; check_step: adam_case_util.meets_the_bars' bars on one network
  Hand, SUITE        one update by hand from the public primitives, holding what a DDPGLearner holds under the same names
  snapshot           every tensor an update writes, as bits
  torch_update, bandit_torch_run   the torch composition: StackedActor under autograd, clip_grad_norm_, torch Adam, foreach Polyak; what
                     it reaches on the bandit

Nothing here imports the native library at import time."""
import copy
import functools
import os
import types

import numpy as np
import torch

import actor_grad_util as U
import actor_ref_util as R
import adam_util as AU
import mlp_grad_util as M
import offpolicy_util as O
import yardstick_util as Y

PARAMS = U.PARAMS
FM, FX = Y.FACTORS
PROFILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "ddpg_float64.json")
# (B, nA, Do, k, central).  The last: 16 385 x 16 = 262 160 elements = 1 025 tiles of 256, the first B at nA = 16 at which a workgroup of
# the head pass takes two tiles (J = 2: 513 workgroups), and the merge's 128 threads per column go round their partial rows five times
SHAPES = ((1, 1, 1, 3, 0), (97, 1, 5, 3, 0), (97, 1, 5, 3, 1), (161, 2, 8, 4, 1), (129, 3, 11, 4, 1), (130, 16, 50, 4, 0), (64, 2, 5, 3, 1),
          (16385, 16, 1, 3, 0))
LARGE = SHAPES[-1]
# the learner's: 1v1, 2v2 and 3v3 at k = 4, then the shapes DDPG is for -- a continuous env (k = 3: the head pads to 4, g_a4's column 3 is
# +0) at 1v1 own and central and at 2v2 central, 4v4 with own critics (Dc = 18), 16 agents with own critics (Do = 50, Dc = 54: the widest
# actor input) and a batch of one row
LEARNER_SHAPES = ((64, 2, 5, 4, 0), (161, 2, 8, 4, 1), (129, 3, 11, 4, 1), (97, 1, 5, 3, 0), (97, 1, 5, 3, 1), (96, 2, 8, 3, 1),
                  (65, 4, 14, 4, 0), (130, 16, 50, 4, 0), (1, 1, 5, 4, 1))
KINK_SHAPES = ((161, 2, 8, 4), (129, 3, 11, 4), (97, 1, 5, 3), (130, 16, 50, 4))
GAMMA = O.GAMMA
# learner_case's generators start here.  Picked on the float64 reference alone: the share of elements the kink filter leaves out moves
# between 0.6 % and 5.7 % from seed to seed (384 hidden values per element, each within 1e-4 of 0 with probability ~1e-4); of the bases
# 0, 10, 20, 30 this is the one at which seeds 0 .. 2 stay under actor_grad_util.KINK_CAP at every shape of KINK_SHAPES (1.0 % .. 4.4 %)
CASE_SEED = 30
# the learner suite's hyper-parameters, and stepped_case's: the same with eps = 1e-3 for both steps.  That eps is a condition, not a
# tuning: Adam's first step is lr g / (|g| + eps), whose slope in g is at most lr / eps.  At eps = 1e-8 a gradient component of the size
# of float32's own error (about 1e-8) moves its parameter by up to lr, and the device's stepped critic and the reference's would
# differ by far more than actor_grad_util.KINK; at eps = 1e-3 a 1e-8 error in g moves a parameter by 2e-8
KW = dict(gamma=GAMMA, tau=0.05, lr_actor=1e-3, lr_critic=2e-3, max_grad_norm=0.5)
STEP_KW = dict(KW, betas=(0.9, 0.999), eps=1e-3)
# stepped_case's seed per shape, 0 where none is given.  Picked on the float64 reference alone, as CASE_SEED was: per shape the first
# seed from 0 at which the kink filter closes within offpolicy_util.MAX_ROUNDS zeroing rounds and leaves out less than actor_grad_util.KINK_CAP.
# Measured (share left out / rounds): 3v3 central 5.68 % / 2 at seed 0 and 4.65 % / 4 at seed 1; 16 agents own 6.25 % / 9 and
# 4.66 % / 4; every other shape passes at seed 0 (0 % .. 4.04 %, 0 .. 2 rounds).  One base for all shapes was looked for first
# (80 bases): the 16-agent shape passes at one base in five (zeroing a row moves its agent's stepped critic by about KINK, so the
# filter closes slowly) and no base passed everywhere.  (96, 2, 8, 3, 1), the 2v2 k = 3 shape, passes at seed 0 as it is
STEP_SEEDS = {(129, 3, 11, 4, 1): 1, (130, 16, 50, 4, 0): 1}
SHARP = ("w1", "w2", "w3", "b3")                     # the tensors the sharpness check of test_ddpg_cpu.py reads


def shape_id(s):
    return "B%d-nA%d-Do%d-k%d-%s" % (*s[:4], "central" if s[4] else "own")


def width(nA, Do, k, central):
    return nA * (Do + k) if central else Do + k


def plan(B, nA):
    """(tiles, tiles per workgroup J, workgroups, rounds of the merge) of bsx_td_head, as the header states them."""
    tiles = -(-B * nA // 256)
    J = -(-tiles // 1024)
    blocks = -(-tiles // J)
    return tiles, J, blocks, -(-blocks // 128)


# ------------------------------------------------------------------------------------------------ the three copies
def join(obs, act, central):
    """obs [B, nA, Do], act [B, nA, k] -> the critic input [B, nA, Dc] (a new array of obs's dtype)."""
    if not central:
        return np.concatenate([obs, act], -1)
    B, nA, _ = obs.shape
    row = np.concatenate([obs.reshape(B, -1), act.reshape(B, -1)], -1)
    return np.repeat(row[:, None, :], nA, axis=1)


def joined(obs, act, central):
    """join as a torch user writes it (any dtype and device, under autograd)."""
    if not central:
        return torch.cat([obs, act], -1)
    B, nA, _ = obs.shape
    return torch.cat([obs.reshape(B, 1, -1), act.reshape(B, 1, -1)], -1).expand(B, nA, -1)


def joined_pi(obs, act, pi, central):
    """x_pi as a torch user writes it: row (b, i) is the replayed joint action with slot i replaced by pi_i(o_i)."""
    if not central:
        return torch.cat([obs, pi], -1)
    B, nA, k = act.shape
    own = torch.eye(nA, dtype=pi.dtype, device=pi.device).view(1, nA, nA, 1)
    actions = own * pi.unsqueeze(1) + (1.0 - own) * act.unsqueeze(1)                  # [B, i, slot, k]
    return torch.cat([obs.reshape(B, 1, -1).expand(B, nA, -1), actions.reshape(B, nA, nA * k)], -1)


def ref_inputs(obs, obs_next, act, central, x_cur, x_next, x_pi):
    """bsx_ddpg_inputs on what the three outputs held before -> new (x_cur, x_next, x_pi)."""
    nA, Do = obs.shape[1:]
    W = nA * Do if central else Do
    cur, nxt = join(obs, act, central), join(obs_next, act, central)
    x_next, x_pi = x_next.copy(), x_pi.copy()
    x_next[..., :W] = nxt[..., :W]
    x_pi[..., :W] = cur[..., :W]
    if central:
        x_pi[..., W:] = cur[..., W:]
    return cur, x_next, x_pi


def ref_put_actions(y4, x, Do, k, central, own_only):
    """bsx_ddpg_put_actions -> a new x."""
    B, nA, _ = y4.shape
    x = x.copy()
    if not central:
        x[..., Do:Do + k] = y4[..., :k]
    elif not own_only:
        x[..., nA * Do:] = y4[:, None, :, :k].reshape(B, 1, nA * k)
    else:
        for i in range(nA):
            x[:, i, nA * Do + i * k:nA * Do + (i + 1) * k] = y4[:, i, :k]
    return x


def ref_action_grad(gx, Do, k, central):
    """bsx_ddpg_action_grad -> g_a4 [B, nA, 4] of gx's dtype; column 3 is +0 with three actions."""
    B, nA, _ = gx.shape
    out = np.zeros((B, nA, 4), gx.dtype)
    for i in range(nA):
        c0 = nA * Do + i * k if central else Do
        out[:, i, :k] = gx[:, i, c0:c0 + k]
    return out


def batch_arrays(shape, seed=0):
    """(obs, obs_next, act) float32 numpy of a shape, standard normals."""
    B, nA, Do, k, _ = shape
    g = np.random.default_rng(100 + seed)
    return tuple(g.standard_normal(s).astype(np.float32) for s in ((B, nA, Do), (B, nA, Do), (B, nA, k)))


# ------------------------------------------------------------------------------------------------ the TD head
def td_inputs(B, nA, seed=0):
    """{q, q_next, rew, weight: float32, done: uint8} CPU tensors [B, nA]: normals, done Bernoulli 0.2, weights uniform in [0.5, 1.5]."""
    g = torch.Generator().manual_seed(8000 + seed + 7 * B + nA)
    rnd = lambda: torch.randn((B, nA), generator=g)           # noqa: E731
    return dict(q=rnd(), q_next=rnd(), rew=rnd(), done=(torch.rand((B, nA), generator=g) < 0.2).to(torch.uint8),
                weight=torch.rand((B, nA), generator=g) + 0.5)


# y = r + gamma (1 - done) Q'(x_next); g_q from the critic's loss, g_pi from -mean w Q; stats[7] = 0
HEAD = O.Head(td_inputs, ("q",), True, lambda f: f["q_next"], lambda t: t["q_next"], "td_head", ("q", "q_next", "rew", "done", "gamma"), PROFILE)


# ------------------------------------------------------------------------------------------------ the learner's case
def ring_rows(N, nA, Do, k, seed=0, done_share=0.2):
    """(obs, act, rew, obs_next, done) of N transitions, CPU float32 / bool: observations and actions uniform in [-1, 1], rewards normal."""
    g = torch.Generator().manual_seed(9000 + seed + 13 * N + nA)
    uni = lambda *s: torch.rand(s, generator=g) * 2 - 1       # noqa: E731
    return uni(N, nA, Do), uni(N, nA, k), torch.randn((N, nA), generator=g), uni(N, nA, Do), torch.rand((N, nA), generator=g) < done_share


def make_nets(nA, Do, k, central, seed=0):
    """(actor, critic) on the CPU: mlp_grad_util.make_net "gains", head weights scaled to sums of order 1 as mlp_grad_util.ddpg_case does."""
    actor, critic = M.make_net(nA, Do, k, "gains", seed + 1), M.make_net(nA, width(nA, Do, k, central), 1, "gains", seed + 2)
    with torch.no_grad():
        critic.w3.mul_(100.0); actor.w3.mul_(60.0)
    return actor, critic


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def joins64(actor, obs, obs_next, act, central, target_actor=None):
    """(x_cur, x_next, x_pi) float64 tensors [B, nA, Dc] of a batch in float64: a' from target_actor (the actor itself if none)."""
    nA, Do = obs.shape[1:]
    k = act.shape[2]
    a64, t64 = R.to_float64(actor), R.to_float64(target_actor if target_actor is not None else actor)
    with torch.no_grad():
        pi, a_next = a64(obs.double()).numpy(), t64(obs_next.double()).numpy()
    o, o2, a = obs.double().numpy(), obs_next.double().numpy(), act.double().numpy()
    pad = lambda y: np.concatenate([y, np.zeros((*y.shape[:2], 4 - k))], -1)       # noqa: E731
    x_cur = join(o, a, central)
    x_next = ref_put_actions(pad(a_next), join(o2, a, central), Do, k, central, False)
    x_pi = ref_put_actions(pad(pi), x_cur, Do, k, central, True)
    return _t(x_cur), _t(x_next), _t(x_pi)


@functools.lru_cache(maxsize=None)
def learner_case(shape, seed=0):
    """(actor, critic, rows, idx, w, share) of a learner shape: the networks, N = 4 B ring rows, the B fixed row indices of the first
    batch, and w [B, nA]: standard normal row weights, 0 where, in float64, a pre-ReLU value is within actor_grad_util.KINK of 0 -- the
    critic's at x_cur and at x_pi, the actor's at obs; share: the part of the elements left out.  Read-only."""
    B, nA, Do, k, central = shape
    seed += CASE_SEED
    actor, critic = make_nets(nA, Do, k, central, seed)
    rows = ring_rows(4 * B, nA, Do, k, seed)
    g = torch.Generator().manual_seed(9500 + seed)
    idx = torch.randint(0, 4 * B, (B,), generator=g)
    obs, act, _, obs_next, _ = (r[idx] for r in rows)
    x_cur, _, x_pi = joins64(actor, obs, obs_next, act, central)
    near = U.near_kink((actor, obs), (critic, x_cur), (critic, x_pi))
    w = torch.randn((B, nA), generator=g)
    w[near] = 0.0
    return actor, critic, rows, idx, w, float(near.double().mean())


def maddpg_grads(actor, critic, batch, w, central, dtype, gamma=GAMMA, target_actor=None, target_critic=None, critic_pi=None):
    """({critic tensor: grad}, {actor tensor: grad}) as float64 arrays, torch autograd on the CPU in `dtype`, of
        critic:  sum_i mean_b w (Q_i(x_cur) - y)^2,  y = r + gamma (1 - done) Q'_i(x_next) held fixed, a' = the target actors' actions
        actor:   sum_i -mean_b w Q_i(x_pi),  x_pi = x_cur with agent i's own action slot replaced by pi_i(o_i)
    batch: (obs, act, rew, obs_next, done) of B rows; the targets default to the networks themselves.  critic_pi: the critic the
    actor's loss reads (an update's stepped critic; networks of any dtype are taken), `critic` itself if none."""
    to = lambda net: U._to(net, "cpu", dtype)                      # noqa: E731
    a, c = to(actor), to(critic)
    c_pi = to(critic_pi) if critic_pi is not None else c
    ta, tc = to(target_actor if target_actor is not None else actor), to(target_critic if target_critic is not None else critic)
    obs, act, rew, obs_next = (t.detach().cpu().to(dtype) for t in (batch[0], batch[1], batch[2], batch[3]))
    notdone, w = 1.0 - batch[4].detach().cpu().to(dtype), w.detach().cpu().to(dtype)
    with torch.no_grad():
        y = rew + gamma * notdone * tc(joined(obs_next, ta(obs_next), central), squash=False)[..., 0]
    critic_loss = (w * (c(joined(obs, act, central), squash=False)[..., 0] - y) ** 2).mean(0).sum()
    gc = torch.autograd.grad(critic_loss, [getattr(c, p) for p in PARAMS])
    actor_loss = -(w * c_pi(joined_pi(obs, act, a(obs), central), squash=False)[..., 0]).mean(0).sum()
    ga = torch.autograd.grad(actor_loss, [getattr(a, p) for p in PARAMS])
    num = lambda gs: {p: g.double().numpy() for p, g in zip(PARAMS, gs)}            # noqa: E731
    return num(gc), num(ga)


# ------------------------------------------------------------------------------------------------ a whole update with distinct targets
def _q_inputs(actor, critic, ta, tc, batch, w, central, dtype):
    """HEAD.ref's inputs of a batch: q = the critic on x_cur and q_next = the target critic on x_next (a' from the target actor),
    both evaluated on the CPU in `dtype`."""
    obs, act, rew, obs_next, done = batch
    to = lambda n: U._to(n, "cpu", dtype)                          # noqa: E731
    with torch.no_grad():
        o, o2, a = obs.to(dtype), obs_next.to(dtype), act.to(dtype)
        q = to(critic)(joined(o, a, central), squash=False)[..., 0]
        q_next = to(tc)(joined(o2, to(ta)(o2), central), squash=False)[..., 0]
    return dict(q=q, q_next=q_next, rew=rew, done=done.to(torch.uint8), weight=w)


def update_reference(actor, critic, ta, tc, batch, w, central, dtype, kw=None, perm=None):
    """One whole update on the CPU in `dtype` (float64: the reference, with adam_mlp_util.reference_step as the two steps; float32:
    the yardstick, torch's own Adam) -> dict(gc, ga: {tensor: grad}; critic, actor: offpolicy_util.first_step's dict; inp: the TD
    head's inputs).  The five parts: the critic's gradient with the target networks in y; the critic's step with its Polyak target; the
    actor's gradient at THAT critic; the actor's step with its target; the TD head's inputs for the statistics.
    perm: the batch's rows in another order (another float32 summation order of the same sums)."""
    kw = kw or STEP_KW
    if perm is not None:
        batch, w = tuple(t[perm] for t in batch), w[perm]
    gc, _ = maddpg_grads(actor, critic, batch, w, central, dtype, kw["gamma"], ta, tc)
    sc, = O.first_step([critic], [gc], [tc], kw["lr_critic"], kw, dtype)
    _, ga = maddpg_grads(actor, critic, batch, w, central, dtype, kw["gamma"], ta, tc, critic_pi=sc["net"])
    sa, = O.first_step([actor], [ga], [ta], kw["lr_actor"], kw, dtype)
    return dict(gc=gc, ga=ga, critic=sc, actor=sa, inp=_q_inputs(actor, critic, ta, tc, batch, w, central, dtype))


def perturbed(net, gen, scale=0.05):
    """A copy of a CPU network with scale * randn added to every parameter."""
    out = R.to_cpu32(net)
    with torch.no_grad():
        for p in PARAMS:
            getattr(out, p).add_(scale * torch.randn(getattr(out, p).shape, generator=gen))
    return out


@functools.lru_cache(maxsize=None)
def stepped_case(shape, seed=None):
    """One update from learner_case's networks, ring rows and idx (at `seed`: STEP_SEEDS' for the shape if none is given) with target networks that are NOT the networks (each parameter plus
    0.05 randn) and STEP_KW's hyper-parameters, on the CPU -> a namespace of
      actor, critic, ta, tc, rows, idx, batch   the starting state (float32, CPU)
      w, share, rounds   the row weights: learner_case's, and 0 also where the STEPPED critic (float64) has a pre-ReLU value within
                         actor_grad_util.KINK of 0 at x_pi -- zeroing rows moves the critic's gradient and so the stepped critic, so the
                         filter is repeated to its fixed point (`rounds` zeroing rounds, at most 4); share: the part left out at the end
      ref, yard          update_reference in float64 and in float32
      stats, e_stats     HEAD.ref's float64 statistics and the float32 yardstick's own error on them over 9 row orders (td_case's)
    Read-only."""
    central = shape[4]
    seed = STEP_SEEDS.get(shape, 0) if seed is None else seed
    actor, critic, rows, idx, w0, _ = learner_case(shape, seed)
    g = torch.Generator().manual_seed(9700 + seed)
    ta, tc = perturbed(actor, g), perturbed(critic, g)
    batch = tuple(r[idx] for r in rows)
    x_pi = joins64(actor, batch[0], batch[3], batch[1], central)[2]
    ref, w, rounds = O.kink_fixed_point(w0, lambda w: update_reference(actor, critic, ta, tc, batch, w, central, torch.float64),
                                        lambda ref: U.near_kink((ref["critic"]["net"], x_pi)))
    assert ref is not None, (shape, seed, rounds)
    yard = update_reference(actor, critic, ta, tc, batch, w, central, torch.float32)
    stats = HEAD.ref(ref["inp"])["stats"]
    return types.SimpleNamespace(seed=seed, actor=actor, critic=critic, ta=ta, tc=tc, rows=rows, idx=idx, batch=batch, w=w, rounds=rounds,
                                 share=float((w == 0).double().mean()), ref=ref, yard=yard, stats=stats,
                                 e_stats=Y.own_error(lambda order: HEAD.autograd(yard["inp"], torch.float32, perm=order), dict(stats=stats), shape[0])[0])


def wrong_variants(case, central):
    """{name: ({tensor: |wrong - right| mean}, {tensor: the yardstick's mean error})} in float64: the critic's gradient with the live
    networks as targets, with the live actor alone, with the live critic alone, and the actor's gradient at the UNSTEPPED critic."""
    c = case
    f = lambda **k: maddpg_grads(c.actor, c.critic, c.batch, c.w, central, torch.float64, STEP_KW["gamma"], **k)     # noqa: E731
    wrong = {"live nets as targets": (f()[0], "gc"), "live actor only": (f(target_critic=c.tc)[0], "gc"),
             "live critic only": (f(target_actor=c.ta)[0], "gc"), "actor at the unstepped critic": (f()[1], "ga")}
    return {name: O.distances(g, c.ref[which], c.yard[which], SHARP) for name, (g, which) in wrong.items()}


def stepped_spread(shape, perms=8):
    """{"gc" / "ga": {tensor: (max ratio, mean ratio)}}: how far the float32 yardstick's own error on the two gradients of stepped_case
    moves when the batch's rows are summed in another order (actor_grad_util.spread over yardstick_util.row_orders).  No kernel output enters."""
    c = stepped_case(shape)
    others = [update_reference(c.actor, c.critic, c.ta, c.tc, c.batch, c.w, shape[4], torch.float32, perm=order)
              for order in list(Y.row_orders(shape[0], perms))[1:]]
    return {which: U.spread(c.ref[which], c.yard[which], [o[which] for o in others]) for which in ("gc", "ga")}


stepped_exceptions = Y.exceptions_from              # {shape id or "*": {"gc" / "ga": {tensor: [fm, fx]}}} from {shape id: stepped_spread's}


def stepped_factor_of(shape, which):
    """name -> (fm, fx) for a gradient of stepped_case: the exception profiles/ddpg_float64.json records (with the spread it came
    from) for the shape or under "*", (2, 4) where it records none."""
    f = Y.recorded(PROFILE, "stepped", "factors")
    return Y.factor_of(f.get(shape_id(shape), {}).get(which, {}), f.get("*", {}))


check_step = AU.check_step


# ------------------------------------------------------------------------------------------------ one update by hand
STATE = ("_blob_a", "_blob_c", "_blob_ta", "_blob_tc", "step_actor", "step_critic", "stats", "step_stats_actor", "step_stats_critic")


def snapshot(x):
    """{name: bits} of everything an update of x (a DDPGLearner or a Hand) writes that outlives it, the ring's draw counter included."""
    torch.cuda.synchronize()
    out = {k: getattr(x, k).detach().clone() for k in STATE}
    out["draws"] = x.buffer._draws.clone()
    for name in ("actor", "critic", "target_actor", "target_critic"):
        for p in PARAMS:
            out[f"{name}.{p}"] = getattr(getattr(x, name), p).detach().view(torch.int32).clone()
    for name in ("adam_actor", "adam_critic"):
        out[name + ".m"], out[name + ".v"] = (t.view(torch.int32).clone() for t in (getattr(x, name).m, getattr(x, name).v))
    return {k: (v.view(torch.int32) if v.dtype == torch.float32 else v.view(torch.int64) if v.dtype == torch.float64 else v) for k, v in out.items()}


class Hand(O.Hand):
    """What a DDPGLearner holds, under the same names, and its update written out with the public primitives alone: offpolicy_util.Hand's
    and ddpg_inputs, td_head.  own_priorities: on a prioritised ring step() also writes the drawn rows' new priorities directly after
    td_head, where DDPGLearner does (tests/test_hip_replay_prio.py hooks them onto td_head instead; td3_util's and sac_util's always do)."""
    own_priorities = False

    def step(self, obs, act, rew, obs_next, done, u, weight=None, adam=True):
        """The ten steps on a batch -> (critic row, actor row): copies of mlp_grad's cached rows."""
        from deep_rl_battlespace_amd import learner as L
        c = self.central
        obs, act, obs_next = obs.contiguous(), act.contiguous(), obs_next.contiguous()
        Do, k = obs.shape[2], act.shape[2]
        x_cur, x_next, x_pi = L.ddpg_inputs(obs, obs_next, act, central=c)
        L.ddpg_put_actions(self.forward(self._blob_ta, obs_next), x_next, Do, k, central=c, own_only=False)
        q_next, q = self.forward(self._blob_tc, x_next, True), self.forward(self._blob_c, x_cur, True)
        head = L.td_head(q, q_next, rew, done, self.gamma, weight=weight)
        self.stats[u].copy_(head.stats)
        if self.prioritized and self.own_priorities:
            self.buffer.update_priorities(q, head.td)
        row_c, = self.critic_rows(x_cur, [head.g_q])
        if adam:
            self.critics_step([row_c], u)
        return row_c, self.deterministic_actor_step(obs, x_pi, head.g_pi, k, u, adam)


SUITE = O.Suite("DDPGLearner", Hand, learner_case, KW)


# ------------------------------------------------------------------------------------------------ the torch composition, the bandit
def torch_update(actor, critic, target_actor, target_critic, opt_a, opt_c, batch, central, gamma=GAMMA, tau=0.01, max_grad_norm=None):
    """One MADDPG update the way a torch user writes it (any device): autograd through StackedActor, clip_grad_norm_, the two Adam
    steps (critic first, the actor against the stepped critic), foreach Polyak."""
    obs, act, rew, obs_next, done = batch
    with torch.no_grad():
        y = rew + gamma * (1.0 - done.to(rew.dtype)) * target_critic(joined(obs_next, target_actor(obs_next), central), squash=False)[..., 0]
    opt_c.zero_grad(set_to_none=True)
    ((critic(joined(obs, act, central), squash=False)[..., 0] - y) ** 2).mean(0).sum().backward()
    if max_grad_norm is not None:
        torch.nn.utils.clip_grad_norm_(critic.parameters(), max_grad_norm)
    opt_c.step()
    opt_a.zero_grad(set_to_none=True)
    (-critic(joined_pi(obs, act, actor(obs), central), squash=False)[..., 0].mean(0).sum()).backward()
    if max_grad_norm is not None:
        torch.nn.utils.clip_grad_norm_(actor.parameters(), max_grad_norm)
    opt_a.step()
    O.polyak_((target_actor, target_critic), (actor, critic), tau)


def bandit_torch_run(N, seed=0):
    """(initial reward, reward after N updates) of the torch composition on offpolicy_util's bandit, on the CPU."""
    b = O.BANDIT

    def compose(seed):
        actor, critic = O.bandit_nets(seed)
        ta, tc = copy.deepcopy(actor), copy.deepcopy(critic)
        oa, oc = torch.optim.Adam(actor.parameters(), lr=b["lr"]), torch.optim.Adam(critic.parameters(), lr=b["lr"])
        return actor, lambda u, batch, g: torch_update(actor, critic, ta, tc, oa, oc, batch, False, tau=b["tau"])
    return O.bandit_torch_run(N, compose, seed)


