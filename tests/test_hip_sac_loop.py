"""The loop of SACLearner's docstring on real rollouts, on the MI355X (tests/offpolicy_loop_util.py's, test_hip_ddpg_loop.py's too): a
continuous env played by PolicyRollout(sample="gaussian") with log_std = log 0.2 in all 2n columns, capture() on an empty ring, then run,
append, update (updates = 2), publish, against an eager twin bit for bit after every iteration.  What only this loop reaches for SAC: a
captured Gaussian rollout reading log_std rows that the learner's Adam step and publish have just written; both draws' sequence word across
graph replays while the ring changes underneath; the learner's graph drawing from a priority tree that an n-step append has just
repaired; a first batch larger than the fill on a prioritised ring; the blue team's columns.  At sigma = 0.2 the Gaussian rollout ends
games inside the rollouts as the DDPG loop's clamped noise of 0.2 does (asserted): the initial log_std is the learner's default."""
import math

import pytest
import torch

import offpolicy_loop_util as L
import sac_util as S

pytestmark = pytest.mark.gpu

# a and c: E T of a rollout is smaller than B (256 against 300, 96 against 129: c's on a prioritised ring).  b: Dc = 2 (8 + 3) = 22, c:
# Dc = 3 (11 + 3) = 42.  seed (40 + n where none is given) and iters: picked on the MI355X so that games end inside the rollouts, finished
# rows reach the head, the ring wraps and, behind a fold, a stored row's window is cut by a game's end -- all asserted;
# profiles/offpolicy_loops.json records what they give
CASES = {
    "a-1v1-one-launch-red-own-3step": dict(n=1, cont=True, one_launch=True, team="red", central=False, E=32, T=8, M=600, B=300, then=False,
                                           iters=6, nstep=3),
    "b-2v2-graph-blue-central-prioritised": dict(n=2, cont=True, one_launch=False, team="blue", central=True, E=24, T=8, M=500, B=161, then=True,
                                                 iters=6, prio=True),
    "c-3v3-one-launch-red-central-prioritised-2step": dict(n=3, cont=True, one_launch=True, team="red", central=True, E=16, T=6, M=400, B=129,
                                                           then=True, iters=8, prio=True, nstep=2),
}


def _log_std(n):
    return torch.full((2 * n, 3), math.log(0.2), device="cuda")


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _twin_publish(hand, tw, cols):
    """The hand's spread into the twin rollout's rows, by hand."""
    with torch.no_grad():
        tw.log_std[cols[0]:cols[0] + len(cols)].copy_(hand.log_std)


def _published(x):
    """The team's rows of the rollout's log_std are the learner's bits and have moved, the other team's are the start's; the policy's
    statistics are finite."""
    mine = x.ro.log_std[x.cols[0]:x.cols[0] + x.n]
    assert _same_bits(mine, x.learner.log_std) and not _same_bits(mine, x.log_std0[x.cols[0]:x.cols[0] + x.n])
    assert _same_bits(x.ro.log_std[x.other], x.log_std0[x.other])
    assert bool(torch.isfinite(x.learner.stats_pi).all())


def _counters(x):
    """Two draws per update and one step of the temperature -- on the learner and on the hand alike."""
    for who in (x.learner, x.hand):
        assert int(who._noise_draws) == 2 * L.UPDATES * x.c.iters and int(who.step_alpha) == L.UPDATES * x.c.iters, who
        assert int(who.step_actor) == L.UPDATES * x.c.iters, who


ALGO = L.Algo("SACLearner", S.Hand, S.snapshot, critics=2, rollout_kw=dict(sample="gaussian", noise_std=0.0, log_std=_log_std),
              twin_publish=_twin_publish, published=_published, at_end=_counters)


@pytest.mark.parametrize("name", list(CASES))
def test_the_documented_loop_equals_its_eager_twin_bit_for_bit(name):
    L.documented_loop(name, CASES[name], ALGO)
