"""CPU-side checks of the centralised PPO critic (learner.joint_width / joint_obs, bsx_ppo_joint_obs, PolicyRollout(central_critic=)):
the numpy restatement of the join (tests/mappo_util.py), which the GPU is held to bit for bit, puts a plane's own observation first
and its team-mates after it in ascending order; the widths and their refusals; the new entry point is declared, bound, exported and
refuses bad sizes before any launch (fake addresses only: no call here reaches a kernel); PolicyRollout validates the new keyword on a
stub env; what the GPU suites' float64 references rest on -- the tied step's group sums on a row made by hand, the critic on the join
against the network written out in numpy, a column permutation as the same function -- and profiles/mappo_wide.json against the rule
that alone may widen a factor."""
import json
import os
import re
import types

import numpy as np
import pytest
import torch

import mappo_util as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _coded(R, n, Do):
    """obs [R, 2n, Do] whose every float encodes (r, plane, column)."""
    r, i, c = np.meshgrid(np.arange(R), np.arange(2 * n), np.arange(Do), indexing="ij")
    return (10000 * r + 100 * i + c).astype(np.float32)


def test_the_join_puts_the_own_observation_first_then_the_team_mates_in_ascending_order():
    # 2v2 by hand: planes 0, 1 are one team, 2, 3 the other; Do = 3
    x = M.join(_coded(2, 2, 3))
    assert x.shape == (2, 4, 6)
    assert x[0].tolist() == [[0, 1, 2, 100, 101, 102], [100, 101, 102, 0, 1, 2], [200, 201, 202, 300, 301, 302], [300, 301, 302, 200, 201, 202]]
    assert x[1, 3].tolist() == [10300, 10301, 10302, 10200, 10201, 10202]
    # 3v3 by hand: the planes each row reads, slot by slot; Do = 2
    x = M.join(_coded(3, 3, 2))
    assert x.shape == (3, 6, 6)
    planes = [[0, 1, 2], [1, 0, 2], [2, 0, 1], [3, 4, 5], [4, 3, 5], [5, 3, 4]]
    for r in range(3):
        for i, order in enumerate(planes):
            assert x[r, i].tolist() == [10000 * r + 100 * j + c for j in order for c in range(2)], (r, i)
    # every size: slot 0 is the plane itself, the others its team in ascending order without it, never the other team
    for n in (1, 2, 3, 4):
        Do = 3 * n + 2
        x = M.join(_coded(5, n, Do)).reshape(5, 2 * n, n, Do)
        plane, col, row = (x.astype(np.int64) // 100) % 100, x.astype(np.int64) % 100, x.astype(np.int64) // 10000
        assert (col == np.arange(Do)).all() and (row == np.arange(5)[:, None, None, None]).all()
        for i in range(2 * n):
            team = i // n
            mates = [j for j in range(team * n, team * n + n) if j != i]
            assert plane[:, i, :, 0].tolist() == [[i] + mates] * 5
    # leading axes are kept, and an int32 view is copied as it is
    bits = np.arange(2 * 3 * 4 * 8, dtype=np.int32).reshape(2, 3, 4, 8)
    assert (M.join(bits).reshape(6, 4, 16) == M.join(bits.reshape(6, 4, 8))).all()


def test_joint_width_is_n_times_the_observation_and_names_the_width_it_refuses():
    from deep_rl_battlespace_amd import learner
    assert [learner.joint_width(n) for n in (1, 2, 3, 4)] == [5, 16, 33, 56]
    assert learner.joint_width(4, 16) == 64 and learner.joint_width(2, 7) == 14
    for n in (0, 5):
        with pytest.raises(ValueError, match=str(n * (3 * n + 2))):
            learner.joint_width(n)
    with pytest.raises(ValueError, match="68"):
        learner.joint_width(4, 17)
    assert "joint_obs" in learner.__doc__ and "central critic" in learner.__doc__
    import deep_rl_battlespace_amd as pkg
    for name in ("joint_obs", "joint_width"):
        assert name in pkg.__all__ and getattr(pkg, name) is getattr(learner, name), name


def test_the_entry_point_is_declared_bound_exported_and_refuses_before_any_launch():
    from deep_rl_battlespace_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "battlespace_hip.h")).read()
    assert re.search(r"^int bsx_ppo_joint_obs\(const float\* obs, int64_t R, int A, int Do, float\* x, void\* stream\);", hdr, flags=re.M)
    assert "bsx_ppo_joint_obs" in _lib.SIGNATURES
    f = _lib.load().bsx_ppo_joint_obs
    ok = 1 << 20                                   # a fake, aligned address: every call below is refused, or has no rows
    assert f(None, 1, 2, 5, ok, None) == -1 and f(ok, 1, 2, 5, None, None) == -1
    assert f(ok, -1, 2, 5, ok, None) == -1 and f(ok, (1 << 30) + 1, 2, 5, ok, None) == -1
    for A in (0, 1, 3, 10, -2):
        assert f(ok, 1, A, 5, ok, None) == -1, A
    assert f(ok, 1, 8, 17, ok, None) == -1 and f(ok, 1, 8, 0, ok, None) == -1 and f(ok, 1, 2, 65, ok, None) == -1
    assert f(ok + 2, 1, 2, 5, ok, None) == -2 and f(ok, 1, 2, 5, ok + 1, None) == -2
    assert f(ok, 0, 8, 14, ok, None) == 0 and f(ok, 0, 2, 64, ok + 4, None) == 0          # no rows: a no-op that succeeds


def _stub_env(n=1, E=8, continuous=False):
    return types.SimpleNamespace(_compat=False, rng="philox", continuous_actions=continuous, n_agents=n, n_envs=E, _A=2 * n,
                                 obs_size=3 * n + 2, device=torch.device("cpu"), env_offset=0)


def test_policy_rollout_validates_the_central_critic_before_any_gpu_call():
    from deep_rl_battlespace_amd.rollout import PolicyRollout, StackedActor
    env, actor = _stub_env(n=2), StackedActor(4, 8, 4)
    central, own = StackedActor(4, 16, 1), StackedActor(4, 8, 1)
    kw = dict(sample="categorical", chains=1, gae=dict(gamma=0.99, lam=0.95))
    with pytest.raises(ValueError, match="excludes value_actor"):
        PolicyRollout(env, actor, 4, central_critic=central, value_actor=own, **kw)
    for bad in (own, StackedActor(4, 16, 4), StackedActor(2, 16, 1), StackedActor(4, 15, 1)):
        with pytest.raises(ValueError, match="central_critic must be a StackedActor"):
            PolicyRollout(env, actor, 4, central_critic=bad, **kw)
    with pytest.raises(ValueError, match="fused"):
        PolicyRollout(env, actor, 4, central_critic=central, fused=False, chains=1)
    with pytest.raises(ValueError, match="85"):
        PolicyRollout(_stub_env(n=5), StackedActor(10, 17, 4), 4, central_critic=StackedActor(10, 85, 1), **kw)
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="central_chunk"):
            PolicyRollout(env, actor, 4, central_critic=central, central_chunk=bad, **kw)
    with pytest.raises(ValueError, match="central_chunk belongs"):
        PolicyRollout(env, actor, 4, value_actor=own, central_chunk=2, **kw)
    with pytest.raises(ValueError, match="value_actor or a central_critic"):
        PolicyRollout(env, actor, 4, sample="categorical", chains=1, gae=dict(gamma=0.99, lam=0.95))
    # accepted in both forms, the one-launch one beyond 1v1 too: value and last_value are views of one [T + 1, E, A] tensor
    for form in (dict(), dict(one_launch=True)):
        ro = PolicyRollout(env, actor, 4, central_critic=central, **kw, **form)
        assert ro._value_w is None and ro.central_critic is central and tuple(ro._central_w.shape) == tuple(central.pack().shape)
        assert tuple(ro.value.shape) == (4, 8, 4) and tuple(ro.last_value.shape) == (8, 4)
        assert ro.value.data_ptr() == ro._values.data_ptr() and ro.last_value.data_ptr() == ro._values[4].data_ptr()
        assert ro.value.is_contiguous() and ro.last_value.is_contiguous() and ro.central_chunk == 5
        assert tuple(ro._central_x.shape) == (5, 8, 4, 16)
    assert PolicyRollout(env, actor, 4, central_critic=central, central_chunk=3, **kw).central_chunk == 3
    assert PolicyRollout(env, actor, 4, central_critic=central, central_chunk=9, **kw).central_chunk == 5
    # the default chunk: the most whole ticks whose input rows stay under the cap, at least one
    big = _stub_env(n=2, E=17000)
    per_tick = 17000 * 4 * 16 * 4
    assert PolicyRollout(big, actor, 16, central_critic=central, **kw).central_chunk == PolicyRollout._CENTRAL_BYTES // per_tick == 7
    # without the keyword nothing of it exists
    ro = PolicyRollout(env, actor, 4, value_actor=own, **kw)
    assert ro._central_w is None and ro.central_critic is None and not hasattr(ro, "_values")


def test_the_tied_references_group_sums_put_every_groups_sum_at_each_of_its_members():
    # four agents in two groups of two, a row of three floats each, by hand; float32 in, float64 out, the input untouched
    row = np.array([[1, 2, 3], [10, 20, 30], [0.5, -1, 4], [0.25, 1, -4]], np.float32)
    kept = row.copy()
    (s,) = M.group_sums([row], 2)
    assert s.dtype == np.float64 and s.tolist() == [[11, 22, 33], [11, 22, 33], [0.75, 0, 0], [0.75, 0, 0]] and (row == kept).all()
    # the sum is taken in float64: 1 + 2^-30 + 2^-30 survives, as it would not in float32
    tiny = np.array([[1.0], [2.0 ** -30], [2.0 ** -30]], np.float32)
    assert M.group_sums([tiny], 3)[0].tolist() == [[1.0 + 2.0 ** -29]] * 3
    # trailing axes of any depth (a w1 of [A, D, 64]), groups of 3 and 4 never mix, g = 1 is the rows themselves
    rng = np.random.default_rng(0)
    for A, g in ((6, 3), (8, 4), (8, 2), (6, 1)):
        w, b = rng.standard_normal((A, 5, 7)).astype(np.float32), rng.standard_normal((A, 3)).astype(np.float32)
        sw, sb = M.group_sums([w, b], g)
        assert sw.shape == w.shape and sb.shape == b.shape
        for a in range(A):
            lo = a // g * g
            assert np.array_equal(sw[a], w[lo:lo + g].astype(np.float64).sum(0)) and np.array_equal(sb[a], b[lo:lo + g].astype(np.float64).sum(0))


def _recorded_stub(n, E=7, T=3, seed=5):
    """What critic_values reads of a rollout: obs [T + 1, E, A, Do] and a central critic at trained weight scale, on the CPU."""
    from deep_rl_battlespace_amd.learner import joint_width
    from deep_rl_battlespace_amd.rollout import StackedActor
    torch.manual_seed(seed)
    critic = StackedActor(2 * n, joint_width(n), 1)
    with torch.no_grad():
        critic.w3.mul_(100.0)
    obs = torch.rand((T + 1, E, 2 * n, 3 * n + 2), generator=torch.Generator().manual_seed(seed)) * 2 - 1
    return types.SimpleNamespace(obs=obs, central_critic=critic)


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_critic_values_is_the_critic_on_the_join_and_a_column_permutation_is_the_same_function(n):
    ro = _recorded_stub(n)
    T1, E, A, Do = ro.obs.shape
    ref, yard = M.critic_values(ro, torch.float64), M.critic_values(ro, torch.float32)
    assert ref.shape == yard.shape == (T1, E, A) and ref.dtype == yard.dtype == np.float64
    # row by row against the network written out in numpy float64 on the join of that row alone
    c = {k: getattr(ro.central_critic, k).detach().double().numpy() for k in M.PARAMS}
    ln = lambda x, g, h: (x - x.mean()) / np.sqrt(x.var() + 1e-5) * g + h     # noqa: E731
    for t, e, a in ((0, 0, 0), (T1 - 1, E - 1, A - 1), (1, 3, n)):
        x = M.join(ro.obs[t, e].double().numpy())[a]
        h = np.maximum(ln(x @ c["w1"][a] + c["b1"][a, 0], c["g1"][a, 0], c["h1"][a, 0]), 0)
        h = np.maximum(ln(h @ c["w2"][a] + c["b2"][a, 0], c["g2"][a, 0], c["h2"][a, 0]), 0)
        assert abs(float(h @ c["w3"][a][:, 0] + c["b3"][a, 0, 0]) - ref[t, e, a]) <= 1e-12 * max(1.0, abs(ref[t, e, a]))
    # permuted alike, float64 agrees to its own rounding and float32 stays a float32 evaluation; the critic itself is left alone
    w1 = ro.central_critic.w1.detach().clone()
    perm = torch.randperm(ro.central_critic.obs_len, generator=torch.Generator().manual_seed(1))
    assert np.abs(M.critic_values(ro, torch.float64, perm) - ref).max() <= 1e-12 * np.abs(ref).max()
    e0, e1 = np.abs(yard - ref).max(), np.abs(M.critic_values(ro, torch.float32, perm) - ref).max()
    assert 0 < e1 < 8 * e0 and e0 < 8 * e1 and e0 < 1e-4 * np.abs(ref).max() and torch.equal(ro.central_critic.w1, w1)
    spread = M.value_yardstick_spread(ro, ref, yard)
    assert len(spread) == 2 and all(1.0 <= s < 8.0 for s in spread), spread


def test_the_profile_records_every_value_case_and_widens_a_factor_only_by_the_rule_on_the_yardsticks_own_spread():
    import yardstick_util as Y
    prof = json.load(open(M.PROFILE))
    assert set(prof["values"]) == set(M.VALUE_CASES) and tuple(prof["factors"]) == Y.FACTORS
    spreads = {case: {"values": rec["yardstick_spread_max_mean"]} for case, rec in prof["values"].items()}
    assert prof["exceptions"] == Y.exceptions_from(spreads)
    for case, rec in prof["values"].items():
        assert Y.within(rec["ratios_mean_max"], M.value_factors(case)), case
    assert M.value_factors("no such case") == Y.FACTORS
