"""The documented loop of the three off-policy learners (DDPGLearner, TD3Learner, SACLearner) on real rollouts, written once:
capture() on an empty ring, then run, append, update, publish, over and over -- against an eager twin (a second env and rollout with
the same seeds, a second ring with the same seed, the update by hand from the public primitives, a publish that copies the parameter
slices and packs afresh), bit for bit after every iteration.  tests/test_hip_ddpg_loop.py, test_hip_td3_loop.py and test_hip_sac_loop.py
keep their case tables and what is their learner's own (an Algo); tests/test_offpolicy_loop_cpu.py checks the tables without a GPU.

  rollout, team_nets, twin_publish, same   the rollout whose games end inside it, the team's networks, the twin's publish, the comparison
  Algo                the learner's class, its Hand and snapshot, the keyword arguments both get, what its rollout needs, its own checks
  documented_loop     the loop of a case -> the case's record (seed, iters, games ended, rows stored, cut windows, sampled finished rows)

With an n-step length > 1 a replay.NStepAppender stands in front of both rings, learner and hand get its bootstrap_gamma, and the
loop's ring and carry are also held to nstep_util.NStepRef + RingRef fed from the rollout's own records (the twin runs the same fold
kernel: twin equality alone says nothing about the fold).  With a prioritised ring the comparison covers leaves, tree, max_priority and
weights, and the tree must be exact after every iteration.

Nothing here imports the native library at import time."""
import gc
import json
import os
import types

import numpy as np
import torch

import ddpg_util as D
import nstep_util as NU
import offpolicy_util as O

GAMMA = O.GAMMA
UPDATES = 2                                         # updates per call of every learner and hand of the loop
RING_FIELDS = ("actor_states", "actor_new_states", "action_mem", "rew_mem", "done_mem")
RECORDS = ("obs", "scores", "rew", "_done", "env_done")
PRIO_FIELDS = ("_leaves", "tree", "max_priority", "weights")
CARRY = (("_c_obs", "c_obs"), ("_c_act", "c_act"), ("_c_rew", "c_rew"), ("_c_done", "c_done"), ("_c_env_done", "c_ed"))
ONE = 65536                                         # a priority of 1.0: max_priority's start
# what a case may leave unsaid: a plain ring, one-step rows, the seed 40 + n
DEFAULTS = dict(precision="f32", then=False, prio=False, nstep=1, seed=None)
RECORDS_ENV = "BSX_LOOP_RECORDS_OUT"                # names a file the cases' records are appended to, one JSON line each


class Algo:
    """A learner as documented_loop takes it.  learner: the class's name in deep_rl_battlespace_amd.learner; Hand, snapshot: its by-hand
    twin and the bits an update leaves; critics: 1 or 2; kw: the keyword arguments learner and hand get beside ddpg_util.KW; rollout_kw:
    what its PolicyRollout gets beside the DDPG loop's (a callable value is called with the team size n, once per rollout);
    twin_publish(hand, tw, cols): what the twin's publish does beyond twin_publish; published(x), at_end(x): the learner's own checks
    after every publish and after the last iteration, x a namespace of the loop's objects."""

    def __init__(self, learner, Hand, snapshot, critics=1, kw=None, rollout_kw=None, twin_publish=None, published=None, at_end=None):
        self.learner, self.Hand, self.snapshot, self.critics = learner, Hand, snapshot, critics
        self.kw, self.rollout_kw = dict(kw or {}), dict(rollout_kw or {})
        self.twin_publish, self.published, self.at_end = twin_publish, published, at_end


def case_of(case):
    """A table row with DEFAULTS filled in -> a namespace."""
    return types.SimpleNamespace(**{**DEFAULTS, **case})


def rollout(n, E, T, cont, one_launch, seed, team="red", precision="f32", **kw):
    """tests/test_hip_replay_device.py's rollout: the other team scripted, head weights x 100 and noise 0.2, so that games end inside
    the rollouts.  team: the side the actor plays.  kw: PolicyRollout's further arguments (noise_std among them)."""
    import deep_rl_battlespace_amd as bsx
    from deep_rl_battlespace_amd import instinct
    from deep_rl_battlespace_amd.rollout import PolicyRollout, StackedActor
    env = bsx.parallel_env(n_agents=n, n_envs=E, seed=seed, auto_reset=True, continuous_actions=cont); env.reset()
    torch.manual_seed(seed)
    actor = StackedActor(2 * n, 3 * n + 2, 3 if cont else 4, device="cuda")
    with torch.no_grad():
        actor.w3.mul_(100.0)
    mine, theirs = (env.possible_red, env.possible_blue) if team == "red" else (env.possible_blue, env.possible_red)
    kw = {"noise_std": 0.2, **{key: (v(n) if callable(v) else v) for key, v in kw.items()}}
    ro = PolicyRollout(env, actor, T, one_launch=one_launch, precision=precision, opponent=instinct.Team(theirs, mine, env), **kw)
    ro.start()
    return env, ro


def team_nets(ro, cols, central, seed, critics=1):
    """(actor, critic[, critic2]) of the team on the GPU: the team's slices of the rollout's actor, and freshly initialised critics."""
    from deep_rl_battlespace_amd.rollout import StackedActor
    n, Do, k = len(cols), ro.actor.obs_len, ro.actor.n_actions
    actor = StackedActor(n, Do, k, device="cuda")
    with torch.no_grad():
        for p in D.PARAMS:
            getattr(actor, p).copy_(getattr(ro.actor, p)[cols[0]:cols[0] + n])
    torch.manual_seed(100 + seed)
    return (actor, *(StackedActor(n, D.width(n, Do, k, central), 1, device="cuda") for _ in range(critics)))


def twin_publish(hand, ro, cols):
    """The ten parameter slices into the rollout's actor, then a fresh pack of the whole actor."""
    with torch.no_grad():
        for p in D.PARAMS:
            getattr(ro.actor, p)[cols[0]:cols[0] + len(cols)].copy_(getattr(hand.actor, p))
    ro.fused.refresh()


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same(what, ro, tw, buf, buf2, learner, hand, snapshot=D.snapshot, apps=None):
    """The loop's side and the twin's hold the same bits: the rollouts' records, the rings (a prioritised ring's leaves, tree,
    max_priority and weights too), what the updates wrote, the packed weights the rollouts play, and the appenders' carry."""
    torch.cuda.synchronize()
    for f in RECORDS + (("logp",) if ro.logp is not None else ()):
        assert torch.equal(getattr(ro, f), getattr(tw, f)), (what, f)
    for f in RING_FIELDS + (PRIO_FIELDS if hasattr(buf, "tree") else ()):
        assert torch.equal(_bits(getattr(buf, f)), _bits(getattr(buf2, f))), (what, f)
    assert buf.mem_cntr == buf2.mem_cntr and torch.equal(buf.last_idx, buf2.last_idx), what
    a, b = snapshot(learner), snapshot(hand)
    assert O.differing(a, b) == [], (what, O.differing(a, b))
    assert torch.equal(ro.fused.weights.view(torch.int32), tw.fused.weights.view(torch.int32)), what
    if apps is not None:
        for f in ("carry_valid",) + tuple(name for name, _ in CARRY):
            assert torch.equal(_bits(getattr(apps[0], f)), _bits(getattr(apps[1], f))), (what, f)


def tree_is_exact(buf, what):
    """A clone of the tree is the tree after rebuild_tree(), and the root is the sum of the leaves."""
    tree = buf.tree.clone()
    buf.rebuild_tree()
    torch.cuda.synchronize()
    leaves = buf._leaves.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    assert torch.equal(tree, buf.tree) and int(buf.tree[-1]) == int(leaves.sum()), what


class _Fold:
    """nstep_util.NStepRef + RingRef fed from the loop's rollout records: the loop's ring, carry_valid and carry tensors after every append."""

    def __init__(self, c, n, Do, k, c0):
        self.n, self.k, self.c0, self.nstep = n, k, c0, c.nstep
        self.ref, self.ring = NU.NStepRef(c.nstep, GAMMA, c.E, n, Do, k), NU.RingRef(c.M, n, Do, k)
        self.cut = 0

    def records(self, ro):
        torch.cuda.synchronize()
        return {key: getattr(ro, name).cpu().numpy() for key, name in (("obs", "obs"), ("act", "scores"), ("rew", "rew"), ("done", "_done"),
                                                                       ("env_done", "env_done"))}

    def check(self, rec, buf, app, what):
        out = self.ref.fold(*NU.team(rec, self.c0, self.n, self.k))
        assert int(buf._stored) == self.ring.append(out, out["skip"]), what
        NU.assert_ring_equal(buf, self.ring, what)
        assert np.array_equal(app.carry_valid.cpu().numpy(), self.ref.valid) and bool(app.carry_valid.all()), what
        for mine, want in CARRY:
            assert np.array_equal(NU.bits(getattr(app, mine).cpu().numpy()), NU.bits(getattr(self.ref, want))), (what, mine)
        self.cut += int(((out["m"] < self.nstep) & (out["skip"] == 0)).sum())      # stored rows whose window a game's end cut


def documented_loop(name, case, algo):
    """The loop of the learners' docstrings for `iters` iterations against its eager twin -> the case's record."""
    from deep_rl_battlespace_amd import learner as LM
    from deep_rl_battlespace_amd import replay
    c = case_of(case)
    n, k, seed = c.n, 3 if c.cont else 4, 40 + c.n if c.seed is None else c.seed
    make = lambda: rollout(n, c.E, c.T, c.cont, c.one_launch, seed, c.team, c.precision, **algo.rollout_kw)     # noqa: E731
    (env, ro), (_, tw), (_, base) = make(), make(), make()                    # the loop's, the twin's, and one that is never published to
    cols = range(n) if c.team == "red" else range(n, 2 * n)
    other = [a for a in range(2 * n) if a not in cols]
    agents = env.possible_red if c.team == "red" else env.possible_blue
    ring = replay.PrioritizedReplayBuffer if c.prio else replay.DeviceReplayBuffer
    buf, buf2 = (ring(c.M, c.B, agents, env.obs_size, env.obs_size * n, k, device="cuda", seed=3) for _ in range(2))
    app = app2 = fold = apps = None
    if c.nstep > 1:
        app, app2 = apps = tuple(replay.NStepAppender(b, c.nstep, GAMMA, c.T, c.E) for b in (buf, buf2))
        fold = _Fold(c, n, env.obs_size, k, cols[0])
        assert app.bootstrap_gamma == float(NU.gamma_chain(GAMMA, c.nstep)[c.nstep]) < GAMMA
    nets = team_nets(ro, cols, c.central, seed, algo.critics)
    # behind a fold both get the appender's gamma^n: the head's one scalar is then the n-step target's
    kw = dict(D.KW, updates=UPDATES, **algo.kw, **({} if app is None else dict(gamma=app.bootstrap_gamma)))
    learner = getattr(LM, algo.learner)(buf, *nets, critic_input="central" if c.central else "own", **kw)
    hand = algo.Hand(buf2, *(O.gpu_copy(net) for net in nets), c.central, **kw)
    snapshot = algo.snapshot
    start = snapshot(learner)
    w0 = ro.fused.weights.clone()
    assert learner.capture() is learner and O.differing(start, snapshot(learner)) == []       # on the empty ring, and it ran nothing
    assert buf.mem_cntr == 0 and O.differing(start, snapshot(hand)) == []
    assert not c.prio or (int(buf.tree[-1]) == 0 and int(buf.max_priority) == ONE)
    source, source2 = (app, app2) if app is not None else (buf, buf2)
    if c.then:
        ro.capture(then=lambda: source.append_rollout(ro, cols))
    else:
        ro.capture()
    x = types.SimpleNamespace(c=c, n=n, cols=cols, other=other, ro=ro, tw=tw, base=base, buf=buf, buf2=buf2, learner=learner, hand=hand, w0=w0,
                              log_std0=None if ro.log_std is None else ro.log_std.clone())

    def loop():
        ro.run()
        if not c.then:
            source.append_rollout(ro, cols)
        learner.update()
        learner.publish(ro, cols)

    def twin():
        tw.run()
        source2.append_rollout(tw, cols)
        hand.update()
        twin_publish(hand, tw, cols)
        if algo.twin_publish is not None:
            algo.twin_publish(hand, tw, cols)

    def published(it):
        """After a publish: the team's rows of the packed weights the rollout plays are the learner's actor's, every other row the start's."""
        torch.cuda.synchronize()
        rows = ro.fused.weights[cols[0]:cols[0] + n]
        assert torch.equal(rows.view(torch.int32), learner._blob_a.view(torch.int32)), it
        assert torch.equal(ro.fused.weights[other].view(torch.int32), w0[other].view(torch.int32)), it
        if algo.published is not None:
            algo.published(x)

    dropped = False
    sampled_done = 0
    for it in range(c.iters - 2):
        loop()
        if fold is not None:
            fold.check(fold.records(ro), buf, app, it)
        twin()
        published(it)
        same(it, ro, tw, buf, buf2, learner, hand, snapshot, apps)
        if c.prio:
            tree_is_exact(buf, it)
        dropped |= bool((ro.env_done[:c.T] != 0).any())
        sampled_done += int(buf._b_done.any(1).sum())
        assert bool(torch.isfinite(learner.stats).all() and torch.isfinite(learner.step_stats_actor).all()
                    and torch.isfinite(learner.step_stats_critic).all()), it
        assert float(learner.stats[1, 0]) == c.B * n
        assert float(learner.stats[1, 5]) == float(buf._b_done.sum()) / (c.B * n)     # the last batch's share of finished rows
        if it == 0:
            kept = int(buf._stored)
            assert 0 < kept == buf.mem_cntr < c.M and int(buf.last_idx.max()) < kept      # drawn from the rows the first rollout left
            assert kept < c.B or c.E * c.T >= c.B                                         # ... a batch larger than the fill
            assert not torch.equal(ro.fused.weights[cols[0]], base.fused.weights[cols[0]])            # publish wrote the team's rows
        if it <= 1:
            # the first tick after the first publish: the same observations and noise keys as a rollout nobody published to, the
            # scripted team's rows the same, the team's rows not -- the captured rollout plays the published actor
            base.run()
            torch.cuda.synchronize()
            assert torch.equal(base.obs[0], ro.obs[0]) and torch.equal(base.scores[0][:, other], ro.scores[0][:, other]), it
            assert torch.equal(base.scores[0][:, list(cols)], ro.scores[0][:, list(cols)]) == (it == 0), it
    del start
    torch.cuda.synchronize()
    gc.collect()                                                              # (as ppo_learner_util.allocates_nothing reads it)
    held = torch.cuda.memory_allocated()
    loop()
    between = fold.records(ro) if fold is not None else None                  # (a copy to the host: the records the second loop overwrites)
    loop()
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == held                              # the loop allocates nothing
    if fold is not None:
        # the first of the two appends against the reference's ring alone: the device ring already holds the second
        out = fold.ref.fold(*NU.team(between, cols[0], n, k))
        fold.ring.append(out, out["skip"])
        fold.cut += int(((out["m"] < c.nstep) & (out["skip"] == 0)).sum())
        fold.check(fold.records(ro), buf, app, "end")
    twin()
    twin()
    published("end")
    same("end", ro, tw, buf, buf2, learner, hand, snapshot, apps)
    dropped |= bool((ro.env_done[:c.T] != 0).any())
    sampled_done += int(buf._b_done.any(1).sum())
    assert dropped                                                            # games ended inside the rollouts: rows were left out
    assert sampled_done > 0                                                   # finished rows reached the TD head
    assert buf.mem_cntr > c.M                                                 # the ring wrapped
    assert int(learner.step_critic) == UPDATES * c.iters == int(buf._draws) == int(hand.step_critic)
    record = dict(learner=algo.learner, case=name, seed=seed, iters=c.iters, games_ended=int(env.counters()[:, 0].sum()), rows_stored=buf.mem_cntr,
                  cut_windows=None if fold is None else fold.cut, sampled_finished_rows=sampled_done)
    if fold is not None:
        assert fold.cut > 0                                                   # a stored row's window was cut by a game's end
    if c.prio:
        tree_is_exact(buf, "end")
        top = int(buf.max_priority) & 0xFFFFFFFF
        leaves = buf.priorities[:c.M].cpu().numpy().astype(np.int64) & 0xFFFFFFFF
        record.update(max_priority=top / ONE, leaves_below_max=int((leaves != top).sum()))
        assert top > ONE                                                      # max_priority has grown beyond its start
        assert (leaves > 0).all() and (leaves != top).any()                   # the learner's priority updates landed between the appends
    if algo.at_end is not None:
        algo.at_end(x)
    print("loop record:", json.dumps(record))
    path = os.environ.get(RECORDS_ENV)
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(record) + "\n")
    return record
