"""The case tables of the three documented-loop suites (tests/test_hip_ddpg_loop.py, test_hip_td3_loop.py, test_hip_sac_loop.py), checked
without a GPU: what the loop of tests/offpolicy_loop_util.py needs of a case before it can assert anything on the device.  Nothing here
imports the native library."""
import pytest

import offpolicy_loop_util as L
import test_hip_ddpg_loop as ddpg
import test_hip_sac_loop as sac
import test_hip_td3_loop as td3

TABLES = {"ddpg": ddpg, "td3": td3, "sac": sac}
MLP_MAX_D = 64                                      # the fused MLP kernels' widest input (learner's _critic_width refuses more)
ALL = [(learner, name) for learner, mod in TABLES.items() for name in mod.CASES]


def _case(learner, name):
    return L.case_of(TABLES[learner].CASES[name])


@pytest.mark.parametrize("learner,name", ALL, ids=["%s-%s" % c for c in ALL])
def test_a_case_fits_the_kernels_wraps_its_ring_and_keeps_the_delay_schedule(learner, name):
    c = _case(learner, name)
    k = 3 if c.cont else 4
    assert c.n >= 1 and c.team in ("red", "blue") and c.precision in ("f32", "bf16x3", "bf16x6")
    if c.central:
        assert c.n * (3 * c.n + 2 + k) <= MLP_MAX_D                           # a central critic's input
    algo = TABLES[learner].ALGO
    assert L.UPDATES % algo.kw.get("policy_delay", 1) == 0                    # a call keeps the schedule
    assert c.E * c.T * c.iters > c.M                                          # the ring can wrap (every row kept; the loop asserts it did)
    assert c.iters >= 3                                                       # iters - 2 compared iterations, then the two that allocate nothing
    assert c.nstep >= 1 and c.T >= c.nstep                                    # a rollout holds a whole window
    assert learner != "sac" or (c.cont and algo.rollout_kw["sample"] == "gaussian")


@pytest.mark.parametrize("learner", list(TABLES))
def test_every_learner_has_a_first_batch_larger_than_the_fill_a_fold_a_prioritised_ring_and_both_together(learner):
    cases = [_case(learner, name) for name in TABLES[learner].CASES]
    assert any(c.E * c.T < c.B for c in cases)
    assert any(c.nstep > 1 for c in cases) and any(c.prio for c in cases) and any(c.nstep > 1 and c.prio for c in cases)
    assert any(c.team == "blue" for c in cases) and any(c.then for c in cases) and any(not c.one_launch for c in cases)


def test_the_ids_are_unique_and_the_ddpg_loops_first_three_are_what_they_were():
    # (a table is a dict literal: a repeated id would silently replace a case, so the counts are checked)
    assert all(" " not in name for mod in TABLES.values() for name in mod.CASES)
    assert list(ddpg.CASES)[:3] == ["1v1-continuous-one-launch-red-own", "2v2-discrete-graph-blue-central", "3v3-discrete-one-launch-red-central"]
    assert len(ddpg.CASES) == 4 and [name[:2] for name in td3.CASES] == ["a-", "b-", "c-"] == [name[:2] for name in sac.CASES]
    names = [learner + "::" + name for learner, name in ALL]
    assert len(set(names)) == len(names)
