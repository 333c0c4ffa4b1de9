"""PolicyRollout(central_critic=) on the MI355X: the value tensor is ONE forward of the critic over the join of all of ro.obs, whatever
the chunking; adv, ret, mask and adv_stats are advantage.gae called by hand on the same records and carry; what was played is what the
same rollout plays with no critic at all; captured and eager runs agree.  T = 4; 1v1 to 4v4; 5 and 96 games; the per-tick graph
and (2v2, 3v3, 4v4: beyond the value head's 1v1) the one-launch form; chunks of 1, 3 (a ragged last chunk) and the default; auto_reset
on and off; a scripted opponent in both forms.  The recorded values -- what GAE and v_old read -- are also held to the critic in float64
on the numpy join, an evaluation that shares nothing with the kernels, at every join width under the project's (2, 4)."""
import numpy as np
import pytest
import torch

import mappo_util as M
import yardstick_util as Y

pytestmark = pytest.mark.gpu

T = 4
# (kind, n, E, one_launch, central_chunk, auto_reset, opponent)
CASES = {
    "categorical-n1-E5-chunk1": ("categorical", 1, 5, False, 1, True, None),
    "categorical-n1-E96-default": ("categorical", 1, 96, False, None, True, None),
    "gaussian-n2-E5-chunk3": ("gaussian", 2, 5, False, 3, True, None),
    "gaussian-n2-E96-default-no_reset": ("gaussian", 2, 96, False, None, False, None),
    "categorical-n2-E96-one_launch-chunk3": ("categorical", 2, 96, True, 3, True, None),
    "categorical-n2-E5-one_launch-default-no_reset": ("categorical", 2, 5, True, None, False, None),
    "gaussian-n2-E96-one_launch-chunk1": ("gaussian", 2, 96, True, 1, True, None),
    "gaussian-n4-E96-chunk1-no_reset": ("gaussian", 4, 96, False, 1, False, None),
    "categorical-n4-E5-default": ("categorical", 4, 5, False, None, True, None),
    "categorical-n4-E96-chunk3": ("categorical", 4, 96, False, 3, True, None),
    "categorical-n2-E96-chunk3-blue_scripted": ("categorical", 2, 96, False, 3, True, "blue"),
    # one launch at every team size it opens (3v3: the join's row of 33 floats is no multiple of four), and with a scripted team in-kernel
    "gaussian-n3-E5-one_launch-chunk3": ("gaussian", 3, 5, True, 3, True, None),
    "categorical-n3-E96-one_launch-default-no_reset": ("categorical", 3, 96, True, None, False, None),
    "categorical-n4-E96-one_launch-chunk1": ("categorical", 4, 96, True, 1, True, None),
    "gaussian-n4-E5-one_launch-default": ("gaussian", 4, 5, True, None, True, None),
    "gaussian-n2-E96-one_launch-default-red_scripted": ("gaussian", 2, 96, True, None, True, "red"),
}
VALUE_CASES, VALUE_E = M.VALUE_CASES, M.VALUE_E


def _bits(x):
    return x.detach().contiguous().view(torch.uint8 if x.element_size() == 1 else torch.int32 if x.element_size() == 4 else torch.int64).cpu()


def _records(ro):
    return [_bits(x) for x in (ro.obs, ro.scores, ro.logp, ro.rew, ro._done, ro.env_done, ro._values, ro.adv, ro.ret, ro._mask, ro.adv_stats,
                               ro._done_prev)]


@pytest.mark.parametrize("case", list(CASES))
def test_values_are_one_forward_over_the_join_gae_is_the_call_by_hand_and_the_critic_is_not_played(case):
    from deep_rl_battlespace_amd import advantage
    kind, n, E, one_launch, chunk, auto_reset, opponent = CASES[case]
    kw = dict(T=T, n=n, E=E, one_launch=one_launch, opponent=opponent, auto_reset=auto_reset, normalize=True, runs=0)
    eager = M.central_rollout(kind, chunk=chunk, capture=False, **kw)
    graph = M.central_rollout(kind, chunk=chunk, capture=True, **kw)
    bare = M.central_rollout(kind, critic=None, capture=True, **kw)
    assert eager.one_launch == one_launch and eager._value_w is None and eager.central_chunk == (chunk or T + 1)
    assert eager.value.data_ptr() == eager._values.data_ptr() and eager.last_value.data_ptr() == eager._values[T].data_ptr()
    g = eager._gae
    for run in range(2):
        carry = eager._done_prev.clone()
        for ro in (eager, graph, bare):
            ro.run()
        torch.cuda.synchronize()
        # captured and eager agree, record by record
        for i, (a, b) in enumerate(zip(_records(eager), _records(graph))):
            assert torch.equal(a, b), (run, i)
        # the critic is not played: the same rollout with no critic at all played the same game
        for name in ("obs", "scores", "logp", "rew", "_done", "env_done"):
            assert torch.equal(_bits(getattr(eager, name)), _bits(getattr(bare, name))), (run, name)
        # ONE forward over the join of all of obs, bit for bit: a forward row does not depend on its neighbours, so the chunks do not show
        assert torch.equal(_bits(eager._values), _bits(M.central_values(eager))), run
        assert bool(torch.isfinite(eager._values).all()) and float(eager._values.abs().max()) > 0
        # advantage.gae by hand on the same records and the carry the run started with
        out = advantage.gae(eager.rew, eager.value, eager.last_value, eager._done, eager.env_done, carry, g["gamma"], g["lam"], normalize=True,
                            agents=eager._gae_agents)
        torch.cuda.synchronize()
        for name, a, b in (("adv", out.adv, eager.adv), ("ret", out.ret, eager.ret), ("mask", out.mask, eager.mask), ("stats", out.stats, eager.adv_stats),
                           ("carry", carry, eager._done_prev)):
            assert torch.equal(_bits(a), _bits(b)), (run, name)
        if opponent is not None:
            cols = eager.opponent._cols
            assert not eager.mask[:, :, cols].any() and bool(eager.mask.any())
    assert bool(eager.mask.any())


@pytest.mark.parametrize("case", list(VALUE_CASES))
def test_the_recorded_values_meet_the_bars_against_the_critic_in_float64_on_the_numpy_join(case):
    """got = ro._values after two captured runs; ref = the critic in float64 torch on the CPU over mappo_util.join(ro.obs), all T + 1
    ticks, at trained weight scale (w3 x 100); yard = the same in float32.  yardstick_util's bars: mean error <= 2x and max error <= 4x
    the yardstick's, unless profiles/mappo_wide.json records an exception that yardstick_util.factor_rule makes of the yardstick's OWN
    spread under column permutations (tests/test_mappo_cpu.py holds the file to that rule).  BSX_MAPPO_RATIOS_OUT names a file the
    measured ratios and spreads are appended to (the profile keeps them)."""
    kind, n, one_launch = VALUE_CASES[case]
    ro = M.central_rollout(kind, T=T, n=n, E=VALUE_E, one_launch=one_launch)
    assert ro.one_launch == one_launch and ro.graph is not None and tuple(ro._values.shape) == (T + 1, VALUE_E, 2 * n)
    got = ro._values.double().cpu().numpy()
    ref, yard = M.critic_values(ro, torch.float64), M.critic_values(ro, torch.float32)
    spread = M.value_yardstick_spread(ro, ref, yard)
    factors = M.value_factors(case)
    print(f"MAPPO values {case}: join width {ro.central_critic.obs_len}, {ref.size} values, max|v| {np.abs(ref).max():.4g}; the yardstick's own "
          f"max / mean error move by {spread[0]:.3f} / {spread[1]:.3f} under 8 column permutations; factors {factors}")
    assert np.isfinite(ref).all() and float(np.abs(ref).max()) > 0.1 and all(e > 0 for e in Y.errors(yard, ref))
    figures, bad = Y.check_tensors([("values", got, ref, yard, factors)], f"MAPPO values {case}", "errors", unit="v")
    M.append_ratios(case, figures["values"][:2], spread)
    assert not bad, (case, figures)
    # what GAE and v_old read are views of that tensor: last_value is its row T; GAE's returns are finite
    assert ro.value.data_ptr() == ro._values.data_ptr() and ro.last_value.data_ptr() == ro._values[T].data_ptr()
    assert torch.equal(_bits(ro.last_value), _bits(ro._values[T])) and torch.equal(_bits(ro.value), _bits(ro._values[:T]))
    assert bool(torch.isfinite(ro.ret).all()) and bool(torch.isfinite(ro.adv).all()) and bool(ro.mask.any())
