"""CPU-side checks of GAE on device (csrc/bsx_advantage.hip, advantage.gae): the numpy restatement (tests/gae_util.py) against a
hand-worked rollout and against the textbook loop; the entry points are declared, exported and bound; every argument the C ABI refuses
is refused before any launch (fake addresses only: no call here gets through to a kernel); PolicyRollout(gae=) needs a value head."""
import ctypes
import inspect
import math
import os
import re
import types

import numpy as np
import pytest
import torch

from gae_util import gae_ref, random_case, textbook_gae

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("bsx_gae_workspace_bytes", "bsx_gae", "bsx_gae_agents")
ARG, ALIGN = -1, -2
P = 4096                      # a 256-byte aligned fake address (never dereferenced)


def _lib():
    from deep_rl_battlespace_amd import _lib
    return _lib


def _worked_example():
    """2 games of 2v2 (A = 4: agents 0, 1 red, 2, 3 blue), T = 6, gamma = lam = 0.5, every value 1, V(obs[T]) = 3.
    Game 0: red agent 0 dies at tick 1 (die_punishment -0.5); a bullet it fired lands at tick 2 (+0.25) and red loses at tick 3, which
    pays it the team's lose_punishment (-1) although it is dead: both are dropped.  Agent 1 gets -1 at tick 3, blue agent 2 +1, agent 3
    a hit at tick 2 (+0.5) and +1 at tick 3.  Tick 4 is the auto-reset re-spawn row (env_done[4] = 1), tick 5 the fresh game's first
    decision, cut off by the rollout's end and bootstrapped from V(obs[T]).
    Game 1: agent 0 was dead before tick 0 (done_prev = 1; an in-flight bullet pays it +0.25 at tick 0: dropped); the game ties at
    tick 1 and stays finished (no auto-reset): ticks 2-5 are inert."""
    T, E, A = 6, 2, 4
    rew = np.zeros((T, E, A), np.float32)
    value = np.ones((T, E, A), np.float32)
    last_value = np.full((E, A), 3.0, np.float32)
    done = np.zeros((T, E, A), np.uint8)
    env_done = np.zeros((T + 1, E), np.uint8)
    done_prev = np.zeros((E, A), np.uint8)
    rew[1, 0, 0] = -0.5
    rew[2, 0, 0] = 0.25
    rew[3, 0, :] = (-1.0, -1.0, 1.0, 1.0)
    rew[2, 0, 3] = 0.5
    done[1:4, 0, 0] = 1
    done[3, 0, :] = 1
    env_done[4, 0] = 1                      # tick 4 found game 0 finished: the re-spawn; done[4] is clear again
    done_prev[1, 0] = 1
    rew[0, 1, 0] = 0.25
    done[:, 1, 0] = 1
    done[1:, 1, :] = 1
    env_done[2:, 1] = 1
    adv = np.array([  # [t][e][a]
        [[-0.875, -0.6875, -0.65625, -0.625], [0.0, -0.75, -0.75, -0.75]],
        [[-1.5, -0.75, -0.625, -0.5], [0.0, -1.0, -1.0, -1.0]],
        [[0.0, -1.0, -0.5, 0.0], [0.0] * 4],
        [[0.0, -2.0, 0.0, 0.0], [0.0] * 4],
        [[0.0] * 4, [0.0] * 4],
        [[0.5] * 4, [0.0] * 4]], np.float32)
    ret = np.array([
        [[0.125, 0.3125, 0.34375, 0.375], [0.0, 0.25, 0.25, 0.25]],
        [[-0.5, 0.25, 0.375, 0.5], [0.0, 0.0, 0.0, 0.0]],
        [[0.0, 0.0, 0.5, 1.0], [0.0] * 4],
        [[0.0, -1.0, 1.0, 1.0], [0.0] * 4],
        [[0.0] * 4, [0.0] * 4],
        [[1.5] * 4, [0.0] * 4]], np.float32)
    mask = np.array([
        [[1, 1, 1, 1], [0, 1, 1, 1]],
        [[1, 1, 1, 1], [0, 1, 1, 1]],
        [[0, 1, 1, 1], [0, 0, 0, 0]],
        [[0, 1, 1, 1], [0, 0, 0, 0]],
        [[0, 0, 0, 0], [0, 0, 0, 0]],
        [[1, 1, 1, 1], [0, 0, 0, 0]]], bool)
    carry = np.array([[0, 0, 0, 0], [1, 1, 1, 1]], np.uint8)
    return (rew, value, last_value, done, env_done, done_prev), (adv, ret, mask, carry)


def test_restatement_matches_the_hand_worked_rollout():
    inputs, (adv, ret, mask, carry) = _worked_example()
    a, r, m, c, stats = gae_ref(*inputs, 0.5, 0.5)
    assert np.array_equal(m, mask)
    assert np.array_equal(a, adv) and np.array_equal(r, ret)
    assert np.array_equal(c, carry) and stats is None
    assert not np.signbit(a[~m]).any() and not np.signbit(r[~m]).any()          # rows that are not decisions: +0
    # the dropped rewards (after death, to a dead team-mate, before tick 0 of a dead agent) change nothing
    rew = inputs[0].copy()
    rew[2, 0, 0] = 7.0; rew[3, 0, 0] = -7.0; rew[0, 1, 0] = 5.0; rew[4, 0, :] = 9.0; rew[2:, 1, :] = 3.0
    a2, r2, m2, _, _ = gae_ref(rew, *inputs[1:], 0.5, 0.5)
    assert np.array_equal(a2, adv) and np.array_equal(r2, ret) and np.array_equal(m2, mask)
    # normalised: masked mean 0 / unbiased std 1 over the 24 decision rows, the others stay 0
    an, rn, _, _, st = gae_ref(*inputs, 0.5, 0.5, normalize=True)
    x = adv[mask].astype(np.float64)
    assert st[0] == mask.sum() == 24 and st[1] == pytest.approx(x.mean(), rel=1e-15) and st[2] == pytest.approx(x.std(ddof=1), rel=1e-15)
    assert np.array_equal(rn, ret) and (an[~mask] == 0).all()
    assert abs(float(an[mask].astype(np.float64).mean())) < 1e-6 and abs(float(an[mask].astype(np.float64).std(ddof=1)) - 1.0) < 1e-6


@pytest.mark.parametrize("T", [1, 2, 5, 32, 100])
def test_restatement_matches_textbook_gae_on_single_episodes(T):
    rng = np.random.default_rng(T)
    for gamma, lam in ((0.99, 0.95), (1.0, 1.0), (0.0, 0.5), (0.9, 0.0)):
        for ends in (False, True):                       # truncated by the rollout's end, or the episode's last tick is terminal
            rew = rng.standard_normal((T, 1, 2)).astype(np.float32)
            value = rng.standard_normal((T, 1, 2)).astype(np.float32)
            lv = rng.standard_normal((1, 2)).astype(np.float32)
            done = np.zeros((T, 1, 2), np.uint8)
            done[T - 1] = ends
            a, r, m, _, _ = gae_ref(rew, value, lv, done, np.zeros((T, 1), np.uint8), np.zeros((1, 2), np.uint8), gamma, lam)
            assert m.all()
            for col in range(2):
                wa, wr = textbook_gae(rew[:, 0, col].astype(np.float64), value[:, 0, col].astype(np.float64), float(lv[0, col]),
                                      done[:, 0, col], gamma, lam)
                np.testing.assert_allclose(a[:, 0, col], wa, rtol=1e-5, atol=1e-5 * (1 + np.abs(wa).max()))
                np.testing.assert_allclose(r[:, 0, col], wr, rtol=1e-5, atol=1e-5 * (1 + np.abs(wr).max()))


@pytest.mark.parametrize("E,A", [(2, 6), (4, 10)])
def test_restatement_matches_textbook_gae_per_column_on_teams_whose_rows_are_no_multiple_of_four(E, A):
    """The shapes at which a lane of the kernel has columns of two games (A = 6, 10 with an even E; tests/test_hip_advantage.py STRADDLE):
    the restatement the kernel is held to, column by column against the textbook loop, each game with its own terminal tick."""
    rng = np.random.default_rng(100 * E + A)
    T, gamma, lam = 9, 0.97, 0.9
    rew, value, lv, _, _, _ = random_case(rng, T, E, A)
    done = np.zeros((T, E, A), np.uint8)
    done[T - 1, ::2] = 1                                 # every other game ends on the last tick, its neighbours are cut off by the rollout's end
    a, r, m, c, _ = gae_ref(rew, value, lv, done, np.zeros((T + 1, E), np.uint8), np.zeros((E, A), np.uint8), gamma, lam)
    assert m.all() and np.array_equal(c, done[T - 1])
    for e in range(E):
        for col in range(A):
            wa, wr = textbook_gae(rew[:, e, col].astype(np.float64), value[:, e, col].astype(np.float64), float(lv[e, col]), done[:, e, col],
                                  gamma, lam)
            np.testing.assert_allclose(a[:, e, col], wa, rtol=1e-5, atol=1e-5 * (1 + np.abs(wa).max()))
            np.testing.assert_allclose(r[:, e, col], wr, rtol=1e-5, atol=1e-5 * (1 + np.abs(wr).max()))
    # a finished game's rows are masked by ITS env_done flag, not its neighbour's: game 0 finished at tick 3 on, game 1 never
    env_done = np.zeros((T + 1, E), np.uint8)
    env_done[3:, 0] = 1
    _, _, m2, _, _ = gae_ref(rew, value, lv, done, env_done, np.zeros((E, A), np.uint8), gamma, lam)
    assert not m2[3:, 0].any() and m2[:3, 0].all() and m2[:, 1:].all()


def test_restatement_normalisation_edge_cases():
    rng = np.random.default_rng(0)
    rew, value, lv, done, env_done, prev = random_case(rng, 4, 3, 2)
    env_done[:] = 1                                     # n = 0: nothing changes, mean = std = 0
    a0, _, _, _, _ = gae_ref(rew, value, lv, done, env_done, prev, 0.9, 0.9)
    a, _, m, _, st = gae_ref(rew, value, lv, done, env_done, prev, 0.9, 0.9, normalize=True)
    assert not m.any() and np.array_equal(st, [0, 0, 0]) and np.array_equal(a, a0)
    env_done[0, 0] = 0                                  # n = 1 (game 0, agent 0, tick 0): std = 0
    prev[:] = 0
    prev[0, 1] = 1
    a, _, m, _, st = gae_ref(rew, value, lv, done, env_done, prev, 0.9, 0.9, normalize=True)
    assert m.sum() == 1 and st[0] == 1 and st[2] == 0 and a[m][0] == 0.0


@pytest.mark.parametrize("T,E,A", [(5, 7, 4), (3, 5, 6)])
def test_restatement_with_agents_flagged_off_gives_them_no_decisions(T, E, A):
    """gae_ref(agents=f): the flagged-on columns are those of the call without the flag (a column's recurrence reads no other column),
    the others are all +0 with mask 0, the carry is every column's, and the normalisation is over the flagged-on masked rows alone."""
    rng = np.random.default_rng(10 * T + A)
    case = random_case(rng, T, E, A, 0.15, 0.1, 0.2)
    plain = gae_ref(*case, 0.97, 0.9)
    irregular = np.array([(7 * a + 3) % 5 < 3 for a in range(A)], np.uint8)
    for f in (np.array([1] * (A // 2) + [0] * (A // 2), np.uint8), np.array([0] * (A // 2) + [1] * (A // 2), np.uint8), irregular):
        on = f.astype(bool)
        assert on.any() and not on.all()
        a, r, m, c, st = gae_ref(*case, 0.97, 0.9, agents=f)
        assert st is None and np.array_equal(c, plain[3])                       # the carry is done[T-1] of every column
        for got, want in ((a, plain[0]), (r, plain[1])):
            assert np.array_equal(got[..., on].view(np.int32), want[..., on].view(np.int32))
            assert (got[..., ~on].view(np.int32) == 0).all()                    # +0 bits
        assert np.array_equal(m[..., on], plain[2][..., on]) and not m[..., ~on].any() and m.any()
        for kernel_order in (False, True):
            an, rn, mn, cn, st = gae_ref(*case, 0.97, 0.9, normalize=True, agents=f, kernel_order=kernel_order)
            x = a[m].astype(np.float64)                                         # the flagged-on masked rows alone
            assert np.array_equal(mn, m) and np.array_equal(rn, r) and np.array_equal(cn, c)
            assert st[0] == m.sum() == x.size < plain[2].sum()
            assert st[1] == pytest.approx(x.mean(), rel=1e-12, abs=1e-15) and st[2] == pytest.approx(x.std(ddof=1), rel=1e-12)
            assert np.array_equal(an[m], ((x - st[1]) / (st[2] + 1e-8)).astype(np.float32)) and (an[~m].view(np.int32) == 0).all()
    # all flags set is no flag
    for got, want in zip(gae_ref(*case, 0.97, 0.9, normalize=True, agents=np.ones(A, np.uint8)), gae_ref(*case, 0.97, 0.9, normalize=True)):
        assert np.array_equal(got, want)


def test_kernel_order_statistics_use_the_kernels_constants_and_stay_numpys_to_rounding():
    import gae_util
    src = open(os.path.join(ROOT, "deep-rl-battlespace_amd", "csrc", "bsx_advantage.hip")).read()
    for name, value in (("WAVE", gae_util.WAVE), ("U", gae_util.U), ("MERGE_TPB", gae_util.MERGE_TPB)):
        m = re.search(r"constexpr int %s = (\d+);" % name, src)
        assert m and int(m.group(1)) == value, name
    rng = np.random.default_rng(5)
    # more than one chunk of ticks, more than one tile of lanes at both widths, more than one round of the merge (> 256 tiles)
    for T, E, A in ((19, 70, 6), (9, 300, 2), (3, 33000, 2)):
        case = random_case(rng, T, E, A)
        case[0][...] += 0.5
        adv, _, mask, _, _ = gae_ref(*case, 0.99, 0.95)
        n, mean, std = gae_util.stats_in_kernel_order(adv, mask)
        x = adv[mask].astype(np.float64)
        assert n == x.size and mean == pytest.approx(x.mean(), rel=1e-12) and std == pytest.approx(x.std(ddof=1), rel=1e-12), (T, E, A)


def test_gae_agents_is_declared_next_to_bsx_gae_and_bsx_gae_is_that_call_without_the_flag():
    hdr = open(os.path.join(ROOT, "include", "battlespace_hip.h")).read()
    m = re.search(r"^int\s+bsx_gae_agents\s*\(([^;]*)\)\s*;", hdr, flags=re.M)
    assert m and "const uint8_t* agent_on" in m.group(1) and "const BsxGaeIo* io" in m.group(1)
    assert hdr.index("int bsx_gae(") < m.start()                               # its contract is written next to bsx_gae's
    L = _lib()
    sig, plain = L.SIGNATURES["bsx_gae_agents"], L.SIGNATURES["bsx_gae"]
    assert sig[0] is plain[0] and sig[1] == plain[1][:1] + [ctypes.c_void_p] + plain[1][1:]     # io, agent_on, then bsx_gae's own
    assert [f for f, _ in L.BsxGaeIo._fields_] == list(IO_FIELDS)               # the struct did not grow: old callers keep working
    from deep_rl_battlespace_amd.advantage import gae
    p = inspect.signature(gae).parameters
    assert p["agents"].kind == p["agents"].KEYWORD_ONLY and p["agents"].default is None
    # refused before any launch like bsx_gae (fake addresses); an agent_on of any alignment is taken
    lib = L.load()
    io = L.BsxGaeIo(*([P] * 9))
    assert lib.bsx_gae_agents(ctypes.byref(io), P + 1, 0, 64, 2, 0.99, 0.95, 0, None, None, None) == ARG
    assert lib.bsx_gae_agents(ctypes.byref(io), P + 1, 8, 64, 3, 0.99, 0.95, 0, None, None, None) == ARG
    assert lib.bsx_gae_agents(None, None, 8, 64, 2, 0.99, 0.95, 0, None, None, None) == ARG
    io.mask = P + 2
    assert lib.bsx_gae_agents(ctypes.byref(io), P + 1, 8, 64, 2, 0.99, 0.95, 0, None, None, None) == ALIGN


def test_gae_symbols_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "battlespace_hip.h")).read()
    declared = set(re.findall(r"^\s*int\s+(bsx_\w+)\s*\(", hdr, flags=re.M))
    lib = _lib().load()
    for name in NAMES:
        assert name in declared and name in _lib().SIGNATURES and hasattr(lib, name), name
    assert lib.bsx_abi_version() == 14                 # additive: the ABI version stays
    import deep_rl_battlespace_amd as bsx
    assert bsx.gae is bsx.advantage.gae and "gae" in bsx.__all__


def test_workspace_bytes():
    lib = _lib().load()
    sz = ctypes.c_size_t()
    # 24 bytes per tile of 64 lanes; a lane owns 4 columns, 2 when E*A is not a multiple of 4
    for (E, A, T), want in (((1, 2, 1), 24), ((128, 2, 32), 24), ((129, 2, 32), 24 * 3), ((65536, 2, 32), 24 * 512), ((65536, 8, 32), 24 * 2048),
                            ((3, 6, 7), 24), ((1 << 30, 32, 1), 24 * (1 << 27))):
        assert lib.bsx_gae_workspace_bytes(E, A, T, ctypes.byref(sz)) == 0 and sz.value == want, (E, A, T)
    for E, A, T in ((0, 2, 1), (-1, 2, 1), ((1 << 30) + 1, 2, 1), (4, 0, 1), (4, 3, 1), (4, 34, 1), (4, 2, 0), (4, 2, 65536)):
        assert lib.bsx_gae_workspace_bytes(E, A, T, ctypes.byref(sz)) == ARG, (E, A, T)
    assert lib.bsx_gae_workspace_bytes(4, 2, 1, None) == ARG


IO_FIELDS = ("rew", "value", "done", "env_done", "last_value", "done_prev", "adv", "ret", "mask")


def test_gae_rejects_bad_arguments_before_any_launch():
    lib = _lib().load()

    def call(io=None, T=8, E=64, A=2, gamma=0.99, lam=0.95, normalize=1, ws=P, stats=P, no_io=False):
        f = dict.fromkeys(IO_FIELDS, P)
        f.update(io or {})
        s = None if no_io else ctypes.byref(_lib().BsxGaeIo(*(f[k] for k in IO_FIELDS)))
        return lib.bsx_gae(s, T, E, A, gamma, lam, normalize, ws, stats, None)

    cases = [(ARG, dict(no_io=True))]
    cases += [(ARG, dict(io={k: None})) for k in IO_FIELDS]
    cases += [(ARG, dict(T=0)), (ARG, dict(T=-1)), (ARG, dict(T=65536))]
    cases += [(ARG, dict(A=0)), (ARG, dict(A=1)), (ARG, dict(A=3)), (ARG, dict(A=-2)), (ARG, dict(A=34))]
    cases += [(ARG, dict(E=0)), (ARG, dict(E=-5)), (ARG, dict(E=(1 << 30) + 1))]
    cases += [(ARG, dict(gamma=1.5)), (ARG, dict(gamma=-0.1)), (ARG, dict(lam=math.nan)), (ARG, dict(gamma=math.nan)), (ARG, dict(lam=1.01)),
              (ARG, dict(gamma=math.inf))]
    cases += [(ARG, dict(normalize=2)), (ARG, dict(normalize=-1)), (ARG, dict(ws=None)), (ARG, dict(stats=None))]
    cases += [(ALIGN, dict(io={k: P + 4})) for k in ("rew", "value", "last_value", "adv", "ret")]
    cases += [(ALIGN, dict(io={k: P + 2})) for k in ("done", "done_prev", "mask")]
    cases += [(ALIGN, dict(ws=P + 4)), (ALIGN, dict(stats=P + 4))]
    # two rules broken at once: every BSX_E_ARG is found before any BSX_E_ALIGN
    cases += [(ARG, dict(io=dict(rew=P + 4), T=0)), (ARG, dict(ws=P + 4, lam=math.nan)), (ARG, dict(io=dict(adv=P + 4), A=3)),
              (ARG, dict(io=dict(mask=P + 1), E=0)), (ARG, dict(stats=P + 4, io=dict(ret=None))), (ARG, dict(io=dict(rew=P + 4, done=None)))]
    for want, kw in cases:
        assert call(**kw) == want, kw


def test_gae_python_surface_validates_before_launch():
    from deep_rl_battlespace_amd.advantage import check_rates, gae
    p = inspect.signature(gae).parameters
    assert list(p)[:8] == ["rew", "value", "last_value", "done", "env_done", "done_prev", "gamma", "lam"]
    assert all(p[k].kind == p[k].KEYWORD_ONLY for k in ("normalize", "out", "stats", "workspace")) and p["normalize"].default is False
    for bad in (1.5, -0.01, math.nan, "x", None):
        with pytest.raises(ValueError):
            check_rates(bad, 0.5)
        with pytest.raises(ValueError):
            check_rates(0.5, bad)
    check_rates(0, 1)
    z = torch.zeros((4, 3, 2))
    with pytest.raises(ValueError):                     # the kernel runs on the GPU only: CPU tensors are refused, not computed here
        gae(z, z, z[0], z.bool(), torch.zeros((5, 3), dtype=torch.uint8), torch.zeros((3, 2), dtype=torch.uint8), 0.9, 0.9)


def _stub_env(n=1, E=8):
    return types.SimpleNamespace(_compat=False, rng="philox", continuous_actions=False, n_agents=n, n_envs=E, _A=2 * n, obs_size=3 * n + 2,
                                 device=torch.device("cpu"), env_offset=0)


def test_policy_rollout_gae_needs_a_value_actor():
    from deep_rl_battlespace_amd.rollout import PolicyRollout, StackedActor
    p = inspect.signature(PolicyRollout.__init__).parameters
    assert "gae" in p and p["gae"].default is None
    env = _stub_env()
    actor = StackedActor(2, 5, 4)
    with pytest.raises(ValueError, match="value_actor"):
        PolicyRollout(env, actor, 4, sample="categorical", chains=1, gae=dict(gamma=0.99, lam=0.95))
    critic = StackedActor(2, 5, 1)
    for bad in (dict(gamma=1.5, lam=0.95), dict(gamma=0.99, lam=math.nan)):
        with pytest.raises(ValueError):
            PolicyRollout(env, actor, 4, sample="categorical", value_actor=critic, chains=1, gae=bad)
