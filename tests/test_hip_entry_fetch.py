"""The per-call two-wave 1v1 kernels' first wave issues its five record and pool loads before anything waits for the kernarg segment
(csrc/bsx_step_split_body.inl): what the wave reads first, and in which order, changed -- what it computes must not have.  The two-wave
kernels against the one-wave kernels (`one_wave=True`) bit for bit, and against the C oracle (tests/fuzz_util.py: the oracle relation of
this suite), at the sizes where a workgroup is ragged: ONE game (one lane pair of the only workgroup; every other lane reads the clamped
last row and stores nothing) and 33 games (a full workgroup and a second one with a single game).  130 calls with auto_reset cross the
time-limit tie of call 121 and the re-spawn behind it.  Every argument the wave fetches is varied: the three action forms, injected
jitter, a non-default reward configuration, the env_done / winner outputs, a game offset (range launches), the argument block of a
captured graph; and the forms that share the argument block (multi-tick launches, the fused rollout) against per-call stepping / the oracle.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

REWARDS = dict(hit_base_reward=131, hit_plane_reward=7, miss_punishment=-3, die_punishment=-8, lose_punishment=-27)
CALLS = 130


def _env(**kw):
    import deep_rl_battlespace_amd as bsx
    return bsx.parallel_env(**kw)


def _same_state(a, b):
    sa, sb = a.export_state(), b.export_state()
    m = sa["bl_live"].bool()
    for k in sa:
        if k in ("bl_x", "bl_y", "bl_dir"):                     # slots without a live bullet hold leftovers
            assert torch.equal(sa["bl_live"], sb["bl_live"]) and torch.equal(sa[k][m], sb[k][m]), k
        else:
            assert torch.equal(sa[k], sb[k]), k


def _actions(enc, T, E, g):
    shoot = torch.rand((T, E, 2), generator=g, device="cuda") < 0.5
    if enc == "cont":
        a = torch.rand((T, E, 2, 3), generator=g, device="cuda", dtype=torch.float32) * 2.6 - 1.3
        a[..., 2] = torch.where(shoot, torch.ones((), device="cuda"), a[..., 2])
        return a
    a = torch.where(shoot, 1, torch.randint(-1, 5, (T, E, 2), generator=g, device="cuda")).to(torch.int32)
    if enc == "scores":
        sc = torch.rand((T, E, 2, 4), generator=g, device="cuda") * 0.5
        sc.scatter_(3, a.clamp(0, 3).long().unsqueeze(-1), 1.0)
        return sc
    return a


@pytest.mark.parametrize("enc", ["int", "scores", "cont"])
@pytest.mark.parametrize("E", [1, 33])
def test_two_wave_per_call_kernel_equals_the_one_wave_kernel_at_ragged_sizes(E, enc):
    """Outputs of every call, the env_done / winner flags after every call and the complete state at the end: identical.  Discrete calls
    carry injected jitter (a non-null `u`), every env a non-default reward configuration."""
    kw = dict(n_agents=1, n_envs=E, seed=23, auto_reset=True, continuous_actions=enc == "cont", **REWARDS)
    a, b = _env(**kw), _env(one_wave=True, **kw)
    oa, ob = a.reset(), b.reset()
    assert all(torch.equal(oa[k], ob[k]) for k in oa)
    g = torch.Generator(device="cuda"); g.manual_seed(11)
    acts = _actions(enc, CALLS, E, g)
    u = torch.rand((CALLS, E, 2), generator=g, device="cuda", dtype=torch.float64) if enc != "cont" else None
    for t in range(CALLS):
        ku = {} if u is None else dict(u=u[t])
        ra, rb = a.step_batch(acts[t], **ku), b.step_batch(acts[t], **ku)
        for x, y, name in zip(ra, rb, ("obs", "rew", "done")):
            assert torch.equal(x, y), (t, name)
        assert torch.equal(a.env_done, b.env_done) and torch.equal(a.winner, b.winner), t
    _same_state(a, b)
    c = a.counters()
    assert (c == b.counters()).all() and int(c[:, 0].sum()) >= E          # every game ended at least once: the tie of call 121 at the latest


def _case(**kw):
    case = dict(n=1, E=33, cont=False, enc="int", form="step", auto_reset=True, host_u=False, wide=False, env_offset=0, seed=4242, T=CALLS, K=10,
                chains=2, p_shoot=0.5, resume=False, rewards=[REWARDS[k] for k in ("hit_base_reward", "hit_plane_reward", "miss_punishment",
                                                                                   "die_punishment", "lose_punishment")])
    case.update(kw)
    return case


ORACLE_CASES = [
    _case(E=1, host_u=True), _case(E=33, host_u=True), _case(E=1, enc="scores"), _case(E=33, enc="scores", env_offset=777),
    _case(E=1, cont=True, enc="f32"), _case(E=33, cont=True, enc="f64"),
    # the same calls from one captured graph (the argument blocks are the graph's own), and as two chains of range launches: a range starts
    # at a whole 256-game block, so 256 + 33 games give the second chain a non-zero game offset and a ragged last workgroup
    _case(E=33, form="graph"), _case(E=1, form="graph", enc="scores"), _case(E=289, form="chains", chains=2),
    _case(E=289, form="chains", chains=2, cont=True, enc="f32"),
]


@pytest.mark.parametrize("case", ORACLE_CASES, ids=lambda c: "E%d-%s-%s%s" % (c["E"], c["enc"], c["form"], "-u" if c["host_u"] else ""))
def test_two_wave_per_call_kernel_vs_c_oracle_at_ragged_sizes(case):
    import fuzz_util
    bad, stats = fuzz_util.run_case(case)
    assert bad is None, (bad, case)
    assert stats["vals"] == CALLS * case["E"] * 2 * 5


@pytest.mark.parametrize("E,n", [(33, 1), (5, 4)])
def test_multi_tick_launch_equals_per_call_stepping(E, n):
    """bsx_step_many_discrete shares the argument block with the per-call kernels: 8 ticks in one launch against 8 calls."""
    T = 8
    kw = dict(n_agents=n, n_envs=E, seed=5, auto_reset=True, **REWARDS)
    a, b = _env(**kw), _env(**kw)
    a.reset(); b.reset()
    g = torch.Generator(device="cuda"); g.manual_seed(2)
    for rep in range(3):
        act = torch.where(torch.rand((T, E, 2 * n), generator=g, device="cuda") < 0.5, 1, torch.randint(0, 4, (T, E, 2 * n), generator=g, device="cuda")).to(torch.int32)
        ra = a.step_many(act, store=True)
        for t in range(T):
            rb = b.step_batch(act[t])
            for x, y, name in zip(ra, rb, ("obs", "rew", "done")):
                assert torch.equal(x[t], y), (rep, t, name)
        assert torch.equal(a.env_done, b.env_done) and torch.equal(a.winner, b.winner)
        _same_state(a, b)


@pytest.mark.parametrize("E,n", [(33, 1), (5, 4)])
def test_fused_rollout_vs_c_oracle(E, n):
    """The fused rollout (T x (actor -> step) in one launch) reads the same argument block: its games replayed by the C oracle."""
    import fuzz_util
    case = dict(form="one_launch", n=n, cont=False, noise="none", opponent="none", precision="f32", auto_reset=True, E=E, T=8, runs=3, chains=2,
                value=False, ou_restart=True, seed=99)
    bad, _ = fuzz_util.run_rollout_case(case)
    assert bad is None, (bad, case)
