"""The loop of TD3Learner's docstring on real rollouts, on the MI355X (tests/offpolicy_loop_util.py's, test_hip_ddpg_loop.py's too):
capture() on an empty ring, then run, append, update, publish, against an eager twin bit for bit after every iteration, with
updates = 2 and policy_delay = 2.  What only this loop reaches for TD3: a captured rollout playing a published TD3 actor after an update
whose delayed half did (the second of each call) and did not (the first) run; the smoothing's sequence word and the delay schedule across
graph replays while the ring changes underneath; the learner's graph drawing from a priority tree that an n-step append has just
repaired; a first batch larger than the fill on a prioritised ring; the blue team's columns through replay.NStepAppender."""
import pytest

import offpolicy_loop_util as L
import td3_util as T

pytestmark = pytest.mark.gpu

UPDATES, POLICY_DELAY = L.UPDATES, 2
# b and c: E T of a rollout is smaller than B (256 against 300, 96 against 129: c's on a prioritised ring).  c: Dc = 3 (11 + 4) = 45.
# seed (40 + n where none is given) and iters: picked on the MI355X so that games end inside the rollouts, finished rows reach the head,
# the ring wraps and, behind a fold, a stored row's window is cut by a game's end -- all asserted; profiles/offpolicy_loops.json records
# what they give
CASES = {
    "a-2v2-discrete-graph-bf16x3-red-central-prioritised": dict(n=2, cont=False, one_launch=False, team="red", central=True, E=24, T=8, M=500,
                                                                B=161, precision="bf16x3", then=True, iters=6, prio=True),
    "b-1v1-continuous-one-launch-blue-own-3step": dict(n=1, cont=True, one_launch=True, team="blue", central=False, E=32, T=8, M=600, B=300,
                                                       precision="f32", then=False, iters=6, nstep=3),
    "c-3v3-discrete-one-launch-red-central-prioritised-2step": dict(n=3, cont=False, one_launch=True, team="red", central=True, E=16, T=6, M=400,
                                                                    B=129, precision="f32", then=True, iters=8, prio=True, nstep=2),
}


def _counters(x):
    """The delayed half ran once per call of two updates, the smoothing drew once per update -- on the learner and on the hand alike."""
    iters = x.c.iters
    for who in (x.learner, x.hand):
        assert int(who.step_critic) == UPDATES * iters and int(who.step_actor) == UPDATES // POLICY_DELAY * iters, who
        assert int(who._noise_draws) == UPDATES * iters, who


ALGO = L.Algo("TD3Learner", T.Hand, T.snapshot, critics=2, kw=dict(policy_delay=POLICY_DELAY), at_end=_counters)


@pytest.mark.parametrize("name", list(CASES))
def test_the_documented_loop_equals_its_eager_twin_bit_for_bit(name):
    L.documented_loop(name, CASES[name], ALGO)
