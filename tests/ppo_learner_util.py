"""What the PPO learner's GPU suites share.

The small rollout (by default the record of tests/test_hip_actor_grad.py's PPO test: n = 1, E = 96, T = 8, the graph form, no opponent,
head weights scaled to trained size), built fresh for each caller: the tests move its networks.

The harness of the update() suites (tests/test_hip_ppo_device_update.py, _shuffle.py, _shared.py; _learner.py takes held, allocates_nothing
and five_calls): KW / STEPS, the one hyper-parameter set; shared / keep / restore, what two learners on one rollout share; everything and
names, one description of all an update moves, in one order; held and allocates_nothing; five_calls and by_hand, the hand-written
sequence at both depths; eager_and_captured, the twin loop; first_step_meets_the_bars; the scripted-opponent bit check."""
import gc

import numpy as np
import torch

import adam_util as U
from actor_grad_util import nudge     # noqa: F401     (the suites' step away from the policy that played, beside the ladder that takes it)

PARAMS = ("w1", "b1", "g1", "h1", "w2", "b2", "g2", "h2", "w3", "b3")
TAU = 0.7
KW = dict(clip=0.2, c_v=0.5, c_e=0.01, vclip=0.2, epochs=2, minibatches=2, max_grad_norm=0.5, lr=1e-3)
HEAD_KW = {k: KW[k] for k in ("clip", "c_v", "c_e", "vclip")}
STEPS = KW["epochs"] * KW["minibatches"]
NO_AGENT_AXIS = ("step", "stats", "step_stats", "shuffle_base", "minibatch_idx")


def small_rollout(kind, gae=True, sample=True, T=8, n=1, E=96, one_launch=False, chains=1, opponent=None, normalize=False, seed=41, runs=2):
    """A captured PolicyRollout with a value head and GAE after `runs` runs: `kind` "gaussian" (continuous env, log_std = -0.5) or
    "categorical" (temperature TAU).  n a side, E games (env seed `seed`), the graph form (over `chains` game ranges) or one launch;
    opponent: None, or "red" / "blue" -- that team is played by the scripted instinct.Team and the actor learns the other;
    normalize: GAE's normalisation."""
    import deep_rl_battlespace_amd as bsx
    from deep_rl_battlespace_amd import instinct
    from deep_rl_battlespace_amd.rollout import PolicyRollout, StackedActor
    A, D = 2 * n, 3 * n + 2
    cont = kind == "gaussian"
    torch.manual_seed(11)
    actor, critic = StackedActor(A, D, 3 if cont else 4, device="cuda"), StackedActor(A, D, 1, device="cuda")
    with torch.no_grad():
        actor.w3.mul_(60.0); critic.w3.mul_(100.0)
    env = bsx.parallel_env(n_agents=n, n_envs=E, seed=seed, auto_reset=True, continuous_actions=cont, device="cuda")
    env.reset()
    kw = {}
    if sample:
        kw = dict(sample="gaussian", log_std=torch.full((A, 3), -0.5, device="cuda")) if cont else dict(sample="categorical", temperature=TAU)
    if opponent is not None:
        mine, theirs = (env.possible_red, env.possible_blue) if opponent == "red" else (env.possible_blue, env.possible_red)
        kw["opponent"] = instinct.Team(mine, theirs, env)
    g = dict(gamma=0.99, lam=0.95, normalize=True) if normalize else dict(gamma=0.99, lam=0.95)
    ro = PolicyRollout(env, actor, T, seed=3, value_actor=critic, gae=g if gae else None, one_launch=one_launch, chains=chains, **kw)
    ro.start(); ro.capture()
    for _ in range(runs):
        ro.run()
    torch.cuda.synchronize()
    return ro


def record(ro, t0=0, t1=None):
    """What a PPO update reads of ticks t0 .. t1 (default: all T) of a rollout's records, on the CPU; a categorical policy's actions as indices."""
    act = ro.scores.clone() if ro.log_std is not None else ro.scores.argmax(-1)
    rec = dict(obs=ro.obs[:ro.T].clone(), act=act, logp=ro.logp.clone(), adv=ro.adv.clone(), ret=ro.ret.clone(), mask=ro.mask.clone())
    return {k: v[t0:t1].cpu() for k, v in rec.items()}


def scripted_columns(n, opponent):
    """(scripted, learned) agent columns of a rollout with opponent "red" / "blue" / None: a team's planes are adjacent columns, red first."""
    red, blue = list(range(n)), list(range(n, 2 * n))
    return {None: ([], red + blue), "red": (red, blue), "blue": (blue, red)}[opponent]


# ---------------------------------------------------------------------------------------------------- what an update moves
def _named_shared(ro):
    """(name, tensor) of what two learners on one rollout share: the parameters, the rollout's two blobs and log_std."""
    out = [(f"{name}.{k}", getattr(net, k)) for name, net in (("actor", ro.actor), ("critic", ro.value_actor)) for k in PARAMS]
    out += [("blob_a", ro.fused.weights), ("blob_v", ro._value_w)]
    return out + ([("log_std", ro.log_std)] if ro.log_std is not None else [])


def _named_moments(learner):
    out = [("m_a", learner.adam_a.m), ("v_a", learner.adam_a.v), ("m_v", learner.adam_v.m), ("v_v", learner.adam_v.v)]
    return out + ([("m_ls", learner.adam_ls.m), ("v_ls", learner.adam_ls.v)] if learner.adam_ls is not None else [])


def _named_own(learner):
    """(name, tensor) of a device_step learner's own state: the moments (log_std's last), the count, both statistics[, the shuffle's]."""
    out = _named_moments(learner) + [("step", learner.step_count), ("stats", learner.stats), ("step_stats", learner.step_stats)]
    return out + ([("shuffle_base", learner.shuffle_base), ("minibatch_idx", learner.minibatch_idx)] if learner.shuffle else [])


def _tensors(pairs):
    return [t for _, t in pairs]


def shared(ro):
    return _tensors(_named_shared(ro))


def moments(learner):
    return _tensors(_named_moments(learner))


def own(learner):
    return _tensors(_named_own(learner))


def names(learner):
    """The names of everything(learner), in its order.  All but NO_AGENT_AXIS have the agent as their leading axis."""
    return [name for name, _ in _named_shared(learner.rollout) + _named_own(learner)]


def keep(ro):
    torch.cuda.synchronize()
    return [t.detach().clone() for t in shared(ro)]


def restore(ro, kept):
    with torch.no_grad():
        for t, k in zip(shared(ro), kept):
            t.copy_(k)


def everything(learner):
    torch.cuda.synchronize()
    return [t.detach().clone() for t in shared(learner.rollout) + own(learner)]


def equal(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and torch.equal(x, y) for x, y in zip(a, b))


def blobs_are_packs(ro):
    return (torch.equal(ro.fused.weights.view(torch.int32), ro.actor.pack().view(torch.int32))
            and torch.equal(ro._value_w.view(torch.int32), ro.value_actor.pack().view(torch.int32)))


def members_are_identical(learner, g):
    """Every member equals its group's leader, bit for bit: parameters, log_std, the rollout's blob rows, the moments."""
    torch.cuda.synchronize()
    for i, t in enumerate(shared(learner.rollout) + moments(learner)):
        v = t.detach().contiguous().view(torch.int32).view(t.shape[0] // g, g, -1)
        if not torch.equal(v, v[:, :1].expand_as(v)):
            return i
    return None


def bits(x, cols):
    return x[cols].contiguous().view(torch.int32)


def scripted_keep_every_bit_and_learned_move(learner, before, after, scripted, learned):
    """before, after: everything(learner) around an update.  Over every tensor with an agent axis, by name."""
    assert len(names(learner)) == len(before) == len(after)
    for name, b, a in zip(names(learner), before, after):
        if name not in NO_AGENT_AXIS:
            assert torch.equal(bits(b, scripted), bits(a, scripted)), name
            assert not torch.equal(bits(b, learned), bits(a, learned)), name


# ---------------------------------------------------------------------------------------------------- allocation
def held(learner):
    """The address of every cached buffer an update touches."""
    from deep_rl_battlespace_amd.learner import _buffers
    out = {("head", R, k): v.data_ptr() for R, b in learner._by_rows.items() for k, v in b.items() if v is not None}
    for net in (learner.actor, learner.critic):
        for key, b in _buffers(net).by_key.items():
            out.update({(id(net), key, k): (v.data_ptr() if v is not None else None) for k, v in b.items()})
    out.update({("shared", i): t.data_ptr() for i, t in enumerate(shared(learner.rollout))})
    if learner.device_step:
        out.update({("own", i): t.data_ptr() for i, t in enumerate(own(learner) + [learner.hyper, learner._adam_ws])})
    if learner.shuffle:
        out.update({("gathered", k): v.data_ptr() for k, v in learner._gathered._asdict().items() if v is not None})
        out.update(shuffle_base=learner.shuffle_base.data_ptr(), minibatch_idx=learner.minibatch_idx.data_ptr())
    return out


def allocates_nothing(learner, warm=True, in_use=True):
    """A second update allocates nothing: the same bytes in use, the same buffers at the same addresses.  warm=False: the learner has
    updated already, the one update here is the measured one.  in_use=False: the addresses alone (the torch-optimiser path)."""
    if warm:
        learner.update()
    torch.cuda.synchronize()
    # (garbage of earlier tests that the collector happens to free during an update would show as a change in memory_allocated)
    gc.collect()
    before, used = held(learner), torch.cuda.memory_allocated()
    learner.update()
    torch.cuda.synchronize()
    assert held(learner) == before
    assert not in_use or torch.cuda.memory_allocated() == used


# ---------------------------------------------------------------------------------------------------- the sequence by hand
def five_calls(ro, kind, mb, blob_a, blob_v, head_kw):
    """One minibatch from the raw calls -- the forward, ppo_head(**head_kw: clip, c_v, c_e, vclip) and both backward calls -- on the
    records `mb` (a learner.Minibatch of R contiguous rows), outputs and buffers of its own -> (actor row, critic row, g_log_std, stats)."""
    from deep_rl_battlespace_amd import _lib
    from deep_rl_battlespace_amd.learner import _actor_forward, _Buffers, _mlp_grad, ppo_head
    lib = _lib.load()
    (R, A, D), dev = mb.obs.shape, mb.obs.device
    y, v = torch.empty((R, A, 4), device=dev), torch.empty((R, A), device=dev)
    _actor_forward(lib, blob_a, mb.obs, y, blob_v, v)
    head = ppo_head(kind, y, v, mb.rec, mb.logp, mb.adv, mb.ret, mb.mask, temperature=TAU if kind == "categorical" else 1.0,
                    log_std=ro.log_std if kind == "gaussian" else None, v_old=mb.value, **head_kw)
    row_a = _mlp_grad(lib, _Buffers().get(R, A, D, dev, lib), blob_a, mb.obs, head.g_pi, True)
    row_v = _mlp_grad(lib, _Buffers().get(R, A, D, dev, lib), blob_v, mb.obs, head.g_v, False)
    return row_a, row_v, head.g_log_std, head.stats


def tick_ranges_of(learner):
    """rows_of for by_hand: step i of an unshuffled update through `learner`.minibatch_grads on the blobs as they stand."""
    span = learner.rollout.T // KW["minibatches"]
    return lambda i: learner.minibatch_grads((i % KW["minibatches"]) * span, (i % KW["minibatches"] + 1) * span, pack=False)


def by_hand(ro, kind, rows_of, group=1):
    """STEPS optimiser steps on the rollout's own blobs: rows_of(i) -> (actor row, critic row, g_log_std, stats), then adam_step(group=)
    from fresh moments and a zero count -> what everything() lists (without the shuffle's two)."""
    from deep_rl_battlespace_amd.learner import AdamState, adam_hyper, adam_step
    nets = [ro.actor, ro.value_actor]
    states = [AdamState(ro.actor), AdamState(ro.value_actor)]
    ls_state = AdamState(ro.log_std) if kind == "gaussian" else None
    hyper, count = adam_hyper(KW["lr"], (0.9, 0.999), 1e-8, KW["max_grad_norm"]), torch.zeros(1, dtype=torch.int64, device="cuda")
    head_rows, step_rows = [], []
    for i in range(STEPS):
        row_a, row_v, g_ls, st = rows_of(i)
        head_rows.append(st.clone())
        step_rows.append(adam_step(nets, [row_a, row_v], states, [ro.fused.weights, ro._value_w], hyper, count,
                                   log_std=ro.log_std if ls_state else None, g_log_std=g_ls, log_std_state=ls_state, group=group).clone())
    return keep(ro) + [states[0].m, states[0].v, states[1].m, states[1].v] + ([ls_state.m, ls_state.v] if ls_state else []) + \
        [count, torch.stack(head_rows), torch.stack(step_rows)]


# ---------------------------------------------------------------------------------------------------- eager and captured twins
def eager_and_captured(ro, make, updates=2, each=None):
    """Twin learners make() on one rollout, one eager, one captured; what they share (parameters, log_std, blobs) is put back between
    their turns, so both take every update from the same state and the same records; a fresh run between updates.
    each(update, graph): the caller's own assertions after an update.  -> (eager, graph, what keep(ro) gave after the last run)."""
    eager, graph = make(), make()
    start, before = keep(ro), everything(graph)
    assert graph.capture() is graph
    assert equal(everything(graph), before) and int(graph.step_count) == 0       # capture() itself moved nothing
    assert not graph.shuffle or int(graph.shuffle_base) == 0
    for update in range(updates):
        eager.update()
        a = everything(eager)
        restore(ro, start)
        graph.update()
        b = everything(graph)
        assert equal(a, b), update
        assert not torch.equal(b[0], start[0]) and blobs_are_packs(ro)
        if each is not None:
            each(update, graph)
        ro.run()                                                                    # fresh records under the updated policy
        start = keep(ro)
    return eager, graph, start


# ---------------------------------------------------------------------------------------------------- the first step, three ways
def first_step_meets_the_bars(ro, kw, reference_step, g=1, norm_rtol=1e-10):
    """One optimiser step from one start state on the same gradient rows and the same (float32-representable) Adam hyperparameters:
    PPOLearner(**kw)'s default path (install + clip_grad_norm_ + torch Adam[, leaders copied over followers]) and its device path,
    both against the float64 restatement reference_step(params, grads, m, v, t, hp) -- the kernel test's bars: mean |error| at most
    2x torch's, maximum at most 4x, pooled per network over the leaders' tensors (every g-th agent).  On both paths every member
    ends equal to its leader."""
    from deep_rl_battlespace_amd.learner import PPOLearner
    hp = U.hyper32(lr=3e-4, max_grad_norm=0.5)
    kw = dict(KW, epochs=1, minibatches=1, lr=hp["lr"], betas=(hp["beta1"], hp["beta2"]), eps=hp["eps"], **kw)
    start = keep(ro)
    device = PPOLearner(ro, device_step=True, **kw)
    rows = [r.clone() if r is not None else None for r in device.minibatch_grads(0, ro.T, pack=False)[:3]]
    nets = (ro.actor, ro.value_actor)
    lead = lambda xs: [np.asarray(x)[::g] for x in xs]     # noqa: E731

    def arrays():
        torch.cuda.synchronize()
        return [U.net_arrays(ro.actor) + [ro.log_std.detach().cpu().numpy().copy()], U.net_arrays(ro.value_actor)]
    p0 = arrays()
    grads = [U.row_to_tensors(rows[0].cpu().numpy(), 3) + [rows[2].cpu().numpy()], U.row_to_tensors(rows[1].cpu().numpy(), 1)]
    flat = lambda groups: [x for grp in groups for x in grp]     # noqa: E731
    zeros = [np.zeros_like(x, dtype=np.float64) for x in flat(p0)]
    P, M, V, t, norm, coef = reference_step(flat(p0), flat(grads), zeros, zeros, 0, hp)
    assert coef < 1.0                                                                # the bound bites: clipping is part of what is compared
    device.update()
    got = arrays()
    got_m = [U.row_to_tensors(device.adam_a.m.cpu().numpy(), 3) + [device.adam_ls.m.cpu().numpy()], U.row_to_tensors(device.adam_v.m.cpu().numpy(), 1)]
    got_v = [U.row_to_tensors(device.adam_a.v.cpu().numpy(), 3) + [device.adam_ls.v.cpu().numpy()], U.row_to_tensors(device.adam_v.v.cpu().numpy(), 1)]
    assert abs(float(device.step_stats[0, 1]) - norm) <= norm_rtol * norm            # (shared: float32 group sums against float64 ones)
    assert members_are_identical(device, g) is None
    restore(ro, start)
    default = PPOLearner(ro, **kw)
    assert all(torch.equal(a, b) for a, b in zip(default.minibatch_grads(0, ro.T)[:3], rows))      # the same gradient rows, bit for bit
    default.update()
    torch.cuda.synchronize()
    assert blobs_are_packs(ro)
    for t_ in shared(ro):                                                            # the torch path ties after its step, before the re-pack
        v = t_.detach().view(t_.shape[0] // g, g, -1)
        assert torch.equal(v, v[:, :1].expand_as(v))
    ref_p, ref_m, ref_v = [P[:11], P[11:]], [M[:11], M[11:]], [V[:11], V[11:]]
    tor = arrays()
    state = lambda key: [[default.optimizer.state[getattr(net, k)][key].cpu().numpy() for k in PARAMS] for net in nets]     # noqa: E731
    tor_m, tor_v = state("exp_avg"), state("exp_avg_sq")
    tor_m[0].append(default.optimizer.state[ro.log_std]["exp_avg"].cpu().numpy())
    tor_v[0].append(default.optimizer.state[ro.log_std]["exp_avg_sq"].cpu().numpy())
    for i in range(2):
        pmv = lambda p, m, v: dict(p=lead(p[i]), m=lead(m[i]), v=lead(v[i]))     # noqa: E731
        U.check_step(pmv(got, got_m, got_v), pmv(ref_p, ref_m, ref_v), pmv(tor, tor_m, tor_v), f"net{i}", names=("p", "m", "v"))
