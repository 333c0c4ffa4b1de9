"""The DQN entry points without a GPU: header, library and binding agree and the ABI version stays; the workspace is bsx_td_head's; every
refusal the header documents comes before any launch, in its stated order (fake addresses); the binding and DQNLearner's constructor
refuse on the host; the numpy restatements of tests/dqn_util.py are what torch float64 autograd of the DQN loss gives (g4 is d loss / d
y4) and their float32 form is a float32 evaluation of the same head; the rows built to hit the corners do hit them; the case tables of the
GPU files are non-empty and the whole-update cases stay under the kink cap on the float64 reference alone; the bandit's torch composition
meets the learning check's condition at the recorded update count; the loop's case is the issue's."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import ddpg_util as D
import dqn_util as Q
import offpolicy_util as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("bsx_dqn_head_workspace_bytes", "bsx_dqn_head")
FIELDS = ("y_cur", "y_next_online", "y_next_target", "act", "rew", "done", "weight", "g4", "q", "td")
OPTIONAL = ("weight", "td")
ARG, ALIGN = -1, -2
A16, A8, A4, A1 = 4096, 4096 + 8, 4096 + 4, 4096 + 1
NAN, INF = float("nan"), float("inf")


def _L():
    from deep_rl_battlespace_amd import _lib
    return _lib


def test_header_library_and_binding_agree_on_the_new_entries_and_the_abi_stays():
    L = _L()
    hdr = open(os.path.join(ROOT, "include", "battlespace_hip.h")).read()
    lib = L.load()
    for name in ENTRIES:
        m = re.search(r"^int\s+%s\s*\(([^;]*)\);" % name, hdr, flags=re.M)
        assert m and name in L.SIGNATURES and hasattr(lib, name), name
        assert len(L.SIGNATURES[name][1]) == m.group(1).count(",") + 1, name
    assert L.ABI_VERSION == 14 == lib.bsx_abi_version() and "#define BSX_ABI_VERSION 14" in hdr
    body = re.search(r"typedef struct BsxDqnIo \{(.*?)\} BsxDqnIo;", hdr, flags=re.S).group(1)
    assert tuple(re.findall(r"(\w+);", body)) == FIELDS == tuple(f for f, _ in L.BsxDqnIo._fields_)
    import deep_rl_battlespace_amd as pkg
    for name in ("DQNLearner", "DQN_STATS", "DqnHead", "dqn_head", "dqn_head_workspace_bytes"):
        assert name in pkg.__all__ and getattr(pkg, name) is getattr(pkg.learner, name), name
    assert pkg.DQN_STATS == ("n",) + Q.STAT_NAMES and len(pkg.DQN_STATS) == 8
    assert pkg.DqnHead._fields == ("g4", "q", "td", "stats")
    # the learner shares DDPGLearner's records, capture, sync and publish: one definition, not a copy
    base = pkg.learner.ddpg._RingLearner
    assert issubclass(pkg.DQNLearner, base) and issubclass(pkg.DDPGLearner, base) and not issubclass(pkg.DQNLearner, pkg.DDPGLearner)
    for name in ("_net", "publish", "capture", "sync", "update", "_net_state"):
        assert getattr(pkg.DQNLearner, name) is getattr(pkg.DDPGLearner, name) is getattr(base, name), name
    doc = pkg.DQNLearner.__doc__
    assert "q_scale >= r_max / (1 - gamma)" in doc and "cannot be reached" in doc and "bootstrap_gamma" in doc and "epsilon-greedy" in doc
    assert "A DQN update:" in pkg.learner.__doc__
    # argmax4 is stated once, and both the step kernels and the head include that statement: the head through bsx_q_head.h, the
    # discrete heads' shared header
    csrc = os.path.join(ROOT, "deep-rl-battlespace_amd", "csrc")
    defs = [f for f in sorted(os.listdir(csrc)) if f.endswith((".h", ".hip", ".inl")) and re.search(r"\bint argmax4\(", open(os.path.join(csrc, f)).read())]
    assert defs == ["bsx_argmax4.h"]
    for f in ("bsx_step_kernel.h", "bsx_q_head.h"):
        assert '#include "bsx_argmax4.h"' in open(os.path.join(csrc, f)).read(), f
    assert '#include "bsx_q_head.h"' in open(os.path.join(csrc, "bsx_dqn_head.hip")).read()


def test_the_workspace_is_bsx_td_heads():
    lib, nb, nb0 = _L().load(), ctypes.c_size_t(), ctypes.c_size_t()
    for B, nA in Q.HEAD_SHAPES + ((64, 2), (512, 2), (65536, 1), (16385, 16), (100000, 7), ((1 << 31) - 1, 16)):
        assert lib.bsx_dqn_head_workspace_bytes(B, nA, ctypes.byref(nb)) == 0 == lib.bsx_td_head_workspace_bytes(B, nA, ctypes.byref(nb0))
        assert nb.value == 64 * D.plan(B, nA)[2] == nb0.value, (B, nA)
    for B_, nA_ in ((0, 2), (1 << 31, 2), (10, 0), (10, 17)):
        assert lib.bsx_dqn_head_workspace_bytes(B_, nA_, ctypes.byref(nb)) == ARG
    assert lib.bsx_dqn_head_workspace_bytes(10, 2, None) == ARG


def test_the_entry_refuses_what_the_header_documents_before_any_launch_in_its_order():
    """Fake addresses only: every call is refused before anything reaches HIP."""
    L = _L()
    lib = L.load()

    def head(B=100, nA=2, gamma=0.95, q_scale=2.0, delta=1.0, double_q=1, mix=0, ws=A16, stats=A16, io=True, **ptr):
        st = L.BsxDqnIo(**{f: ptr.get(f, None if f in OPTIONAL else A16) for f in FIELDS})
        return lib.bsx_dqn_head(ctypes.byref(st) if io else None, B, nA, gamma, q_scale, delta, double_q, mix, ws, stats, None)

    required = [f for f in FIELDS if f not in OPTIONAL + ("y_next_online",)]
    for kw in [dict(io=False), dict(ws=None), dict(stats=None)] + [{f: None} for f in required] + \
            [dict(gamma=-0.01), dict(gamma=1.01), dict(gamma=NAN), dict(gamma=INF), dict(B=0), dict(B=1 << 31), dict(nA=0), dict(nA=17)] + \
            [dict(q_scale=0.0), dict(q_scale=-1.0), dict(q_scale=NAN), dict(delta=-0.5), dict(delta=NAN)] + \
            [dict(double_q=2), dict(double_q=-1), dict(mix=2), dict(mix=-1), dict(y_next_online=None)]:
        assert head(**kw) == ARG, kw
    for kw in [{f: A4} for f in ("y_cur", "y_next_online", "y_next_target", "act", "g4")] + [{f: A8} for f in ("y_cur", "act", "g4")] + \
            [{f: A1} for f in ("rew", "weight", "q", "td")] + [dict(ws=A4), dict(stats=A4), dict(y_next_online=A4, double_q=0)]:
        assert head(**kw) == ALIGN, kw
    # argument rules come before alignment rules, whichever pointer is off
    for kw in (dict(g4=A4, gamma=2.0), dict(ws=A4, B=0), dict(y_cur=A4, q_scale=0.0), dict(act=A1, delta=-1.0), dict(q=A1, mix=3),
               dict(rew=A1, y_next_online=None), dict(stats=A4, double_q=5)):
        assert head(**kw) == ARG, kw
    # done at any byte; y_next_online may be NULL without double Q; delta = 0 and the ends of [0, 1] are in: the call gets as far as the
    # alignment rules
    assert head(g4=A4, done=A1, gamma=0.0, delta=0.0) == ALIGN and head(g4=A4, gamma=1.0, double_q=0, y_next_online=None, delta=INF) == ALIGN


def test_the_binding_and_the_learners_constructor_refuse_on_the_host():
    from deep_rl_battlespace_amd import learner as L
    from deep_rl_battlespace_amd.replay import DeviceReplayBuffer
    from deep_rl_battlespace_amd.rollout import StackedActor
    r4, r2, flag = torch.zeros((4, 2, 4)), torch.zeros((4, 2)), torch.zeros((4, 2), dtype=torch.uint8)
    with pytest.raises(ValueError, match="GPU"):
        L.dqn_head(r4, r4, r4, r2, flag, 0.9, q_scale=2.0)
    with pytest.raises(ValueError, match=r"y_cur must be a float32 \[B, nA, 4\] tensor"):
        L.dqn_head(r2, r4, r4, r2, flag, 0.9, q_scale=2.0)
    for kw, match in ((dict(q_scale=0.0), "q_scale"), (dict(q_scale=NAN), "q_scale"), (dict(q_scale=2.0, huber_delta=-1.0), "huber_delta"),
                      (dict(q_scale=2.0, mix="qmix"), "mix must be")):
        with pytest.raises(ValueError, match=match):
            L.dqn_head(r4, r4, r4, r2, flag, 0.9, **kw)
    with pytest.raises(ValueError, match="DeviceReplayBuffer"):
        L.DQNLearner(object(), None, q_scale=2.0)
    with pytest.raises(TypeError):                                   # q_scale has no default: the bound of Q is the caller's choice
        L.DQNLearner(object(), None)
    four = DeviceReplayBuffer(64, 16, list(range(2)), 8, 16, 4, device="cpu")
    three = DeviceReplayBuffer(64, 16, list(range(2)), 8, 16, 3, device="cpu")
    net = StackedActor(2, 8, 4)
    with pytest.raises(ValueError, match="n_actions == 4"):
        L.DQNLearner(three, StackedActor(2, 8, 3), q_scale=2.0)
    for bad in (StackedActor(2, 8, 3), StackedActor(2, 9, 4), StackedActor(3, 8, 4), object()):
        with pytest.raises(ValueError, match="qnet must be a StackedActor"):
            L.DQNLearner(four, bad, q_scale=2.0)
    for kw, match in ((dict(mix="qmix", q_scale=2.0), "mix must be"), (dict(q_scale=0.0), "q_scale"), (dict(q_scale=-3.0), "q_scale"),
                      (dict(q_scale=2.0, huber_delta=-1.0), "huber_delta"), (dict(q_scale=2.0, gamma=1.5), "gamma"),
                      (dict(q_scale=2.0, updates=0), "updates")):
        with pytest.raises(ValueError, match=match):
            L.DQNLearner(four, net, **kw)
    with pytest.raises(ValueError):                                  # the fused MLP's own checks follow: a CPU ring has nothing to run on
        L.DQNLearner(four, net, q_scale=2.0)


def test_the_split_and_large_head_shapes_get_the_plans_they_are_chosen_for():
    """dqn_util.PLANS on host arithmetic alone: per shape the workspace holds one partial row of 64 bytes per workgroup, a workgroup
    takes J = ceil(tiles / workgroups) tiles, and at least two rows lie across a tile edge (none at nA = 16, which divides 256); the large forms give every template bit
    both values; J = 2 and J = 3 are both there, and the last workgroup of (87382, 3) has two live threads and a tile past `tiles`."""
    from deep_rl_battlespace_amd import learner
    assert set(Q.PLANS) == set(Q.SPLIT_SHAPES + Q.LARGE_SHAPES) and not set(Q.PLANS) & set(Q.HEAD_SHAPES)
    for (B, nA), (tiles, J, groups) in Q.PLANS.items():
        nbytes = learner.dqn_head_workspace_bytes(B, nA)
        assert nbytes % 64 == 0 and nbytes // 64 == groups == D.plan(B, nA)[2], (B, nA)
        assert tiles == -(-B * nA // Q.TILE) and -(-tiles // groups) == J == -(-tiles // Q.MAX_BLOCKS), (B, nA)
        split = Q.split_rows(B, nA)
        if Q.TILE % nA:
            assert len(split) >= 2 and (nA != 3 or split[:2].tolist() == [85, 170]), (B, nA)
        else:                                                                       # 16 divides 256: TD3's shape is there for J = 2 at the widest team
            assert (B, nA) == (16385, 16) and len(split) == 0
        print("B%d-nA%d: %d tiles, J = %d, %d workgroups, %d split rows" % (B, nA, tiles, J, groups, len(split)))
    assert [Q.PLANS[s][1] for s in Q.SPLIT_SHAPES] == [1, 1] and sorted({Q.PLANS[s][1] for s in Q.LARGE_SHAPES}) == [2, 3]
    assert all(not len(Q.split_rows(B, nA)) for B, nA in Q.HEAD_SHAPES)             # what the older shapes never reach
    B, nA = Q.LARGE_SHAPES[0]
    tiles, J, groups = Q.PLANS[(B, nA)]
    assert B * nA - (tiles - 1) * Q.TILE == 2 and groups * J == tiles + 1
    assert 171 * 3 == 2 * Q.TILE + 1 and Q.B_SPLIT == 171 and Q.TEAMS[2][0] == 3
    for bit in range(4):
        assert len({bool(f[bit]) if bit else f[bit] for f in Q.LARGE_FORMS}) == 2, bit
    assert set(Q.LARGE_FORMS) <= set(Q.FORMS) and Q.LARGE_PERMS == 2
    assert len(Q.head_cases()) == len({Q.head_case_id(c) for c in Q.head_cases()}) == 6 * 16 + 3 * 4


@pytest.mark.parametrize("form", Q.FORMS, ids=Q.form_id)
@pytest.mark.parametrize("BnA", Q.HEAD_SHAPES + Q.SPLIT_SHAPES, ids=lambda s: "B%d-nA%d" % s)
def test_the_restatement_is_float64_autograd_of_the_dqn_loss(BnA, form):
    """ref64 against torch float64 autograd from the tanh rows: g4 equals d loss / d y4, q and td the composition's, the statistics its
    means; contract32, operation by operation in float32, is a float32 evaluation of the same head."""
    mix, dbl, delta, w = form
    kw = dict(delta=delta, double=dbl, mix=mix, weight=w)
    inp = Q.head_inputs(*BnA)
    ref, t64, c32 = Q.ref64(inp, **kw), Q.torch_head(inp, torch.float64, **kw), Q.contract32(inp, **kw)
    for k in ("g4", "q", "td"):
        err = float(np.abs(ref[k] - t64[k]).max() / np.abs(t64[k]).max())
        assert err <= 1e-12, (k, err)
        assert c32[k].dtype == np.float32 and np.abs(c32[k] - ref[k]).max() <= 1e-5 * max(1.0, np.abs(ref[k]).max()), k
    assert ref["stats"][0] == t64["stats"][0] == inp["rew"].numel()
    for i in range(1, 8):
        assert abs(ref["stats"][i] - t64["stats"][i]) <= 1e-12 * max(abs(t64["stats"][i]), 1e-300), i
    a = inp["act"].argmax(-1).numpy()
    assert ((ref["g4"] != 0).sum(-1) <= 1).all() and (np.take_along_axis(ref["g4"], a[..., None], -1)[..., 0] != 0).mean() > 0.9
    if mix == "vdn":
        assert all((ref[k] == ref[k][:, :1]).all() for k in ("q", "td"))
    if delta and BnA[0] > 100:
        inside = np.abs(ref["q"] - ref["td"]) <= delta
        assert inside.any() and not inside.all()                      # both sides of the Huber corner
        assert mix == "vdn" or 0.05 < inside.mean() < 0.95            # (a team's summed error is seldom within 1)


GAMMA32 = float(np.float32(Q.GAMMA))


@pytest.mark.parametrize("BnA", Q.HEAD_SHAPES, ids=lambda s: "B%d-nA%d" % s)
def test_the_corner_rows_hit_the_corners_they_are_built_for(BnA):
    B, nA = BnA
    inp, fitted = Q.corner_inputs(B, nA)
    assert fitted == tuple(c for r, c in enumerate(Q.CORNERS) if r < B and not (r == 10 and nA == 1)) and len(fitted) >= 1
    if B < len(Q.CORNERS):
        return
    for mix in Q.MIXES:
        for delta in (0.0, Q.DELTA):
            c = Q.contract32(inp, delta=delta, mix=mix)
            d = c["q"] - c["td"]
            col = lambda b, i=0: int(np.flatnonzero(c["g4"][b, i] != 0)[0])         # noqa: E731
            assert col(0) == 1 and col(3) == 2                                      # the first maximum; a NaN is the maximum
            assert np.isnan(c["g4"][7]).sum() == nA and np.isnan(c["td"][7]).sum() == 0 and np.isnan(d[7]).all()     # a NaN d stays
            assert np.isfinite(c["td"][5]).all() and np.isfinite(c["td"][6]).all()          # finished rows keep NaN and inf out
            assert d[8, 0] == 1.0 and d[9, 0] == -1.0                               # |d| exactly delta
            if delta:                                                               # the corner itself is not clipped: the slope of d^2
                assert c["g4"][8, 0, 1] == np.float32(2.0 / B) * np.float32(Q.Q_SCALE) == -c["g4"][9, 0, 1]
            if nA > 1:
                assert inp["done"][10, 0] == 1 and inp["done"][10, 1] == 0 and np.isfinite(c["td"][10]).all()
            assert col(11) == 0                                                     # four equal scores: the first
            if mix == "vdn":
                assert all(np.array_equal(c[k].view(np.int32), np.repeat(c[k][:, :1], nA, 1).view(np.int32)) for k in ("q", "td"))
    # double Q picks by the online rows -- ties and NaN by argmax4's rule -- and values by the target rows
    c = Q.contract32(inp, double=True)
    assert c["td"][1, 0] == np.float32(GAMMA32 * np.float64(Q.Q_SCALE * -0.5) + np.float64(inp["rew"][1, 0]))
    assert c["td"][4, 0] == np.float32(GAMMA32 * np.float64(Q.Q_SCALE * 0.25) + np.float64(inp["rew"][4, 0]))
    assert np.isnan(Q.contract32(inp, double=False)["td"][4, 0])                    # the target's own NaN is its maximum


def test_the_case_tables_are_non_empty_and_the_whole_update_cases_stay_under_the_kink_cap():
    """The GPU files' tables; and per (team, mix) the float64 reference ALONE leaves out at most a quarter of the rows at the case's
    seed -- the first from 0 that qualifies --, closes within offpolicy_util.MAX_ROUNDS, and no arg-max margin lies below KINK."""
    assert len(Q.HEAD_SHAPES) == 4 and len(Q.FORMS) == 16 and len(set(Q.FORMS)) == 16 and len(Q.CORNERS) == 12
    assert Q.TEAMS == ((1, 5), (2, 8), (3, 11), (16, 50)) and Q.B == 64 and Q.MIXES == ("independent", "vdn")
    assert Q.STEP_CASES[:8] == tuple((t, m, Q.B) for t in Q.TEAMS for m in Q.MIXES) and Q.STEP_CASES[8:] == tuple(((3, 11), m, 171) for m in Q.MIXES)
    rec = json.load(open(Q.PROFILE))
    assert set(rec["stepped"]["cases"]) == {Q.team_id(*c) for c in Q.STEP_CASES}
    for team, mix, batch in Q.STEP_CASES:
        sid = Q.team_id(team, mix, batch)
        for s in range(Q.step_seed(team, mix, batch)):
            assert Q.try_seed(team, mix, s, batch)[0] is None, (sid, s)
        c = Q.stepped_case(team, mix, batch)
        print(sid, f"seed {c.seed}: left out {100 * c.share:.2f} % of the rows after {c.rounds} rounds; smallest margin {c.margin:.2e}")
        assert c.share <= Q.KINK_CAP and c.rounds <= O.MAX_ROUNDS and c.margin >= Q.KINK
        assert c.w.shape == (batch, team[0]) == c.batch[2].shape and c.B == batch
        assert not (Q.near_kink(c.qnet, c.batch, c.ref, mix) & (c.w != 0)).any()
        assert float((c.w != 0).double().mean()) >= 0.75 and not torch.equal(c.target.w1, c.qnet.w1)
        assert c.ref["net"]["coef"] < 1.0                                         # the clip is active
        assert not bool(c.batch[4].all()) and bool(c.batch[4].any())
        r = rec["stepped"]["cases"][sid]
        assert r["seed"] == c.seed and abs(r["left_out_percent"] - 100 * c.share) <= 0.005 + 1e-9 and r["zeroing_rounds"] == c.rounds
        for name, (mean, mx) in rec["stepped"]["kernel"].get(sid, {}).items():
            assert mean <= Q.Y.FACTORS[0] and mx <= Q.Y.FACTORS[1], (sid, name)
    assert "factors" not in rec or rec["factors"] == {}                           # nothing is held to a wider factor than (2, 4)


def test_the_bandits_torch_composition_learns_the_paying_arm_at_the_recorded_update_count():
    """The learning check's condition, on the composition alone: after BANDIT['N'] updates the float32 twin's greedy action is the
    paying arm on every probe observation (|o_0| >= MARGIN), for both mixes; so is the float64 twin's."""
    b = Q.BANDIT
    rows, probe = Q.bandit_rows()
    assert float(probe[..., 0].abs().min()) >= b["MARGIN"] - 1e-7 and 0.2 < float(rows[2].mean()) < 0.3 and bool(rows[4].all())
    assert 1.0 / (1.0 - 0.0) <= b["q_scale"]                                      # one-step rows: r_max = 1 bounds Q
    for mix in Q.MIXES:
        draws = Q.bandit_draws(b["N"])
        net, losses = Q.bandit_twin(mix, draws, torch.float32)
        net64, losses64 = Q.bandit_twin(mix, draws, torch.float64)
        print(mix, f"N = {b['N']}: loss {losses[0]:.4f} -> {losses[-1]:.3e} (float64 {losses64[-1]:.3e})")
        assert Q.greedy_is_best(net, probe) and Q.greedy_is_best(net64, probe) and losses[-1] < 0.05 * losses[0]
        assert not Q.greedy_is_best(Q.bandit_qnet(), probe)


def test_the_loops_case_is_the_issues():
    c = Q.LOOP
    assert (c["n"], c["E"], c["T"], c["nstep"], c["iters"], c["noise_std"], c["M"]) == (2, 64, 8, 3, 3, 0.3, 4096)
    assert c["E"] * c["T"] >= c["B"] and c["mixes"] == Q.MIXES and c["updates"] >= 1
