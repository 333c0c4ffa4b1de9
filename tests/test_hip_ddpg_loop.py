"""The loop of DDPGLearner's docstring on real rollouts, on the MI355X: capture() on an empty ring, then run, append_rollout, update,
publish, over and over -- against an eager twin (a second env and rollout with the same seeds, a second ring with the same seed, the
update by hand from the public primitives, a publish that copies the parameter slices and packs afresh), bit for bit after every
iteration.  What only this loop reaches: a captured rollout replaying with published weights (blob rows copied in place under a frozen
pointer, the bfloat16 terms of the 64 x 64 layer included), the learner's graph reading a ring the append kernels of the same stream
have just written, a first batch larger than the ring's fill, the blue team's columns, and capture() before the first row exists.  The
loop itself is tests/offpolicy_loop_util.py's, shared with test_hip_td3_loop.py and test_hip_sac_loop.py; the last case puts an n-step
fold and a prioritised ring behind it."""
import pytest

import ddpg_util as D
import offpolicy_loop_util as L

pytestmark = pytest.mark.gpu

# 1v1 and 3v3: E T of a rollout is smaller than B, so the first batches are larger than the ring's fill (2v2: 192 rows against 161).
# iters: enough for the ring to wrap (asserted).  The last: replay.NStepAppender (n = 3) in front of a PrioritizedReplayBuffer -- the
# appender's max-priority leaves and range repair interleave with the learner graph's clear, max and by-row repair on one stream
CASES = {
    "1v1-continuous-one-launch-red-own": dict(n=1, cont=True, one_launch=True, team="red", central=False, E=32, T=8, M=600, B=300,
                                              precision="f32", then=False, iters=6),
    "2v2-discrete-graph-blue-central": dict(n=2, cont=False, one_launch=False, team="blue", central=True, E=24, T=8, M=500, B=161,
                                            precision="bf16x3", then=True, iters=6),
    "3v3-discrete-one-launch-red-central": dict(n=3, cont=False, one_launch=True, team="red", central=True, E=16, T=6, M=400, B=129,
                                                precision="f32", then=False, iters=8),
    "2v2-discrete-graph-red-central-prioritised-3step": dict(n=2, cont=False, one_launch=False, team="red", central=True, E=24, T=8, M=500,
                                                             B=161, precision="f32", then=True, iters=6, prio=True, nstep=3),
}
_rollout, _team_nets = L.rollout, L.team_nets


class _Hand(D.Hand):
    own_priorities = True                     # on a prioritised ring the hand writes the rows' new priorities where DDPGLearner does


ALGO = L.Algo("DDPGLearner", _Hand, D.snapshot)


@pytest.mark.parametrize("name", list(CASES))
def test_the_documented_loop_equals_its_eager_twin_bit_for_bit(name):
    L.documented_loop(name, CASES[name], ALGO)


def test_publish_and_append_refuse_another_teams_columns_and_another_action_count():
    from deep_rl_battlespace_amd.learner import DDPGLearner
    from deep_rl_battlespace_amd.replay import DeviceReplayBuffer
    env, ro = _rollout(2, 8, 2, False, False, 7)                              # 2v2 discrete: 4 env columns, 4 actions
    buf = DeviceReplayBuffer(64, 16, env.possible_red, env.obs_size, env.obs_size * 2, 4, device="cuda")
    actor, critic = _team_nets(ro, range(2), True, 7)
    learner = DDPGLearner(buf, actor, critic)
    ro.run()
    for cols in (range(1), range(3), range(4), [0, 2], range(3, 5)):          # a 1v1 team's, a 3v3 team's, both teams', a gap, past the end
        with pytest.raises(ValueError, match="contiguous range"):
            learner.publish(ro, cols)
        with pytest.raises(ValueError, match="contiguous range"):
            buf.append_rollout(ro, cols)
    assert buf.mem_cntr == 0
    _, cont = _rollout(2, 8, 2, True, False, 7)                               # the same env, continuous: an actor of 3 actions
    with pytest.raises(ValueError, match="4 actions"):
        learner.publish(cont, range(2))
    learner.publish(ro, range(2, 4))                                          # the blue columns take a team of the same shape
    assert int(buf.append_rollout(ro, range(2)).item()) > 0
