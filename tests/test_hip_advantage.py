"""GAE on the MI355X (csrc/bsx_advantage.hip, advantage.gae, PolicyRollout(gae=)): bit for bit the numpy restatement of
tests/gae_util.py on random records of every shape class (teams up to 16 a side; lanes whose 4 columns lie in two games), normalised to the restatement's float64 statistics, the same bits on every
call and graph replay, nothing written outside the outputs; inside a rollout, computed from the rollout's own records without
disturbing them."""
import numpy as np
import pytest
import torch

from gae_util import gae_ref, random_case

pytestmark = pytest.mark.gpu

GUARD = 256                  # sentinel elements after every output


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _guarded(shape, dtype, fill):
    """A tensor of `shape` that is the head of a larger buffer; the GUARD elements behind it hold `fill`."""
    n = int(np.prod(shape))
    buf = torch.full((n + GUARD,), fill, dtype=dtype, device="cuda")
    return buf, buf[:n].view(shape)


def _run(case, gamma, lam, normalize=False, agents=None):
    """bsx_gae (bsx_gae_agents with `agents`) on a case (numpy arrays) with guarded outputs -> (adv, ret, mask, done_prev', stats) on the host."""
    from deep_rl_battlespace_amd.advantage import gae
    rew, value, lv, done, env_done, prev = case
    T, E, A = rew.shape
    bufs = [_guarded((T, E, A), torch.float32, 7.0), _guarded((T, E, A), torch.float32, 7.0), _guarded((T, E, A), torch.uint8, 0xAB)]
    pbuf, p = _guarded((E, A), torch.uint8, 0xCD)
    p.copy_(_dev(prev))
    kw = {} if agents is None else dict(agents=_dev(agents))
    r = gae(_dev(rew), _dev(value), _dev(lv), _dev(done), _dev(env_done), p, gamma, lam, normalize=normalize, out=tuple(b[1] for b in bufs), **kw)
    torch.cuda.synchronize()
    for (buf, _), fill in zip(bufs, (7.0, 7.0, 0xAB)):
        assert (buf[-GUARD:] == fill).all(), "write past the end of an output"
    assert (pbuf[-GUARD:] == 0xCD).all(), "write past the end of done_prev"
    return (r.adv.cpu().numpy(), r.ret.cpu().numpy(), r.mask.cpu().numpy(), p.cpu().numpy(),
            None if r.stats is None else r.stats.cpu().numpy())


def _assert_exact(got, want, what):
    a, r, m, c = got[:4]
    wa, wr, wm, wc = want[:4]
    assert np.array_equal(m, wm), (what, "mask", int((m != wm).sum()))
    assert np.array_equal(a.view(np.int32), wa.view(np.int32)), (what, "adv", int((a.view(np.int32) != wa.view(np.int32)).sum()))
    assert np.array_equal(r.view(np.int32), wr.view(np.int32)), (what, "ret")
    assert np.array_equal(c, wc), (what, "done_prev")


# (E, A).  A lane owns 4 adjacent columns of a tick's E*A where E*A is a multiple of 4, else 2.  With 4, a lane's columns lie in TWO games
# (the kernel's e0 / e1 / split, env_done read per column) exactly where A is no multiple of 4: A = 6, 10, 14, .. with an even E.  STRADDLE
# are those shapes; (3, 32) is the widest team at 4 columns (never across a game), (33, 10) and (77, 6) take 2 columns.
STRADDLE = [(2, 6), (64, 6), (66, 10), (6, 14), (4, 22), (2, 26)]
assert all(E * A % 4 == 0 and A % 4 != 0 for E, A in STRADDLE)
SHAPES = [(1, 2), (3, 2), (63, 2), (64, 2), (65, 4), (127, 2), (257, 8), (1000, 4), (77, 6)] + STRADDLE + [(3, 32), (33, 10)]
assert (3 * 32) % 4 == 0 and 32 % 4 == 0 and (33 * 10) % 4 != 0


@pytest.mark.parametrize("T", [1, 2, 7, 32, 129])
def test_gae_is_bit_identical_to_the_restatement(T):
    rng = np.random.default_rng(T)
    for E, A in SHAPES:
        for p_done, p_env, p_prev in ((0.1, 0.1, 0.2), (0.02, 0.0, 0.0), (0.5, 0.5, 0.5)):
            case = random_case(rng, T, E, A, p_done, p_env, p_prev)
            gamma, lam = float(rng.uniform(0.8, 1.0)), float(rng.uniform(0.5, 1.0))
            _assert_exact(_run(case, gamma, lam), gae_ref(*case, gamma, lam), (T, E, A, p_done))
    case = random_case(rng, T, 33, 2)
    for gamma, lam in ((0.0, 0.0), (1.0, 1.0), (0.0, 1.0), (1.0, 0.0)):         # the ends of the range
        _assert_exact(_run(case, gamma, lam), gae_ref(*case, gamma, lam), (T, gamma, lam))


def test_gae_full_size_1v1_is_bit_identical():
    rng = np.random.default_rng(7)
    case = random_case(rng, 32, 65536, 2, 0.03, 0.03, 0.05)
    _assert_exact(_run(case, 0.99, 0.95), gae_ref(*case, 0.99, 0.95), "65536 x 1v1")


def _assert_normalised(got, want, what):
    a, r, m, c, st = got
    wa, wr, wm, wc, wst = want
    assert np.array_equal(m, wm) and np.array_equal(c, wc), what
    assert np.array_equal(r.view(np.int32), wr.view(np.int32)), (what, "ret is not normalised")
    assert (a[~m] == 0).all(), what
    assert (np.abs(a.astype(np.float64) - wa) <= 1e-6 * (1 + np.abs(wa))).all(), (what, float(np.abs(a - wa).max()))
    assert st[0] == wst[0], (what, st, wst)
    for i in (1, 2):
        assert abs(st[i] - wst[i]) <= 1e-12 * max(abs(wst[i]), 1e-300) or st[i] == wst[i], (what, i, st, wst)


def test_normalised_advantages_and_stats_match_the_restatement():
    rng = np.random.default_rng(11)
    for T, E, A in ((1, 5, 2), (7, 63, 2), (32, 257, 8), (129, 100, 4), (32, 65536, 2), (32, 64, 6), (7, 6, 10)):
        case = random_case(rng, T, E, A)
        case[0][...] += 0.5                                                      # a mean well away from 0: the 1e-12 bound is relative
        _assert_normalised(_run(case, 0.99, 0.95, True), gae_ref(*case, 0.99, 0.95, True), (T, E, A))
    case = random_case(rng, 4, 9, 2)
    case[4][:] = 1                                                               # no decision row: n = 0, nothing changes
    _assert_normalised(_run(case, 0.9, 0.9, True), gae_ref(*case, 0.9, 0.9, True), "n = 0")
    case[4][0, 0] = 0
    case[5][:] = 0
    case[5][0, 1] = 1                                                            # one decision row: std = 0
    got = _run(case, 0.9, 0.9, True)
    assert got[2].sum() == 1 and got[4][0] == 1 and got[4][2] == 0 and got[0][got[2]][0] == 0.0


def test_two_calls_and_graph_replays_give_the_same_bits():
    from deep_rl_battlespace_amd.advantage import gae, workspace_bytes
    rng = np.random.default_rng(3)
    T, E, A = 32, 4099, 4
    rew, value, lv, done, env_done, prev = (_dev(x) for x in random_case(rng, T, E, A))
    p = prev.clone()
    adv, ret, mask = torch.empty_like(rew), torch.empty_like(rew), torch.empty((T, E, A), dtype=torch.uint8, device="cuda")
    stats = torch.zeros(3, dtype=torch.float64, device="cuda")
    ws = torch.empty(workspace_bytes(E, A, T), dtype=torch.uint8, device="cuda")

    def call():
        p.copy_(prev)
        gae(rew, value, lv, done, env_done, p, 0.97, 0.9, normalize=True, out=(adv, ret, mask), stats=stats, workspace=ws)

    outs = []
    for _ in range(2):
        call()
        torch.cuda.synchronize()
        outs.append([x.clone() for x in (adv, ret, mask, p, stats)])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for _ in range(2):
        for x in (adv, ret, stats):
            x.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        outs.append([x.clone() for x in (adv, ret, mask, p, stats)])
    for o in outs[1:]:
        for x, y in zip(outs[0], o):
            assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))


# ---- inside a rollout


def _actors(n, seed=5):
    from deep_rl_battlespace_amd.rollout import StackedActor
    torch.manual_seed(seed)
    A, D = 2 * n, 3 * n + 2
    actor, critic = StackedActor(A, D, 4, device="cuda"), StackedActor(A, D, 1, device="cuda")
    with torch.no_grad():
        actor.w3.mul_(60.0); critic.w3.mul_(100.0)                                 # decisive policies: planes die, games end early
    return actor, critic


def _rollout(n, E, T, one_launch, chains, actor, critic, gae=None, then=None):
    import deep_rl_battlespace_amd as bsx
    from deep_rl_battlespace_amd.rollout import PolicyRollout
    env = bsx.parallel_env(n_agents=n, n_envs=E, seed=41, auto_reset=True, device="cuda")
    env.reset()
    ro = PolicyRollout(env, actor, T, seed=3, one_launch=one_launch, chains=chains, sample="categorical", temperature=0.7, value_actor=critic,
                       gae=gae)
    ro.start()
    ro.capture(then=None if then is None else (lambda: then(ro)))
    return env, ro


RECORDS = ("obs", "scores", "logp", "value", "rew", "_done", "env_done")


@pytest.mark.parametrize("n,E,one_launch,chains", [(1, 301, False, 1), (1, 512, False, 2), (2, 256, False, 1), (2, 512, False, 2),
                                                   (1, 301, True, 1)])
def test_rollout_gae_equals_the_restatement_of_its_own_records(n, E, one_launch, chains):
    from deep_rl_battlespace_amd.rollout import FusedActor
    T, runs, gamma, lam = 32, 5, 0.99, 0.95                                        # 160 ticks: past the time-limit tie (121 at 1v1)
    actor, critic = _actors(n)
    _, ro = _rollout(n, E, T, one_launch, chains, actor, critic, gae=dict(gamma=gamma, lam=lam))
    _, plain = _rollout(n, E, T, one_launch, chains, actor, critic)
    assert ro.chains == plain.chains == chains
    side = FusedActor(actor, n, seed=99)
    lv_scores, lv = torch.empty((E, 2 * n, 4), device="cuda"), torch.empty((E, 2 * n), device="cuda")
    prev = ro._done_prev.clone()
    assert not prev.any()                                                          # seeded from the env after reset()
    ends = carried = 0
    for k in range(runs):
        ro.run(); plain.run()
        torch.cuda.synchronize()
        for f in RECORDS:                                                          # the extra passes disturb nothing
            assert torch.equal(getattr(ro, f), getattr(plain, f)), (k, f)
        side.forward_into(ro.obs[T], lv_scores, 0.0, seq=1234, value=dict(weights=critic.pack(), out=lv))
        assert torch.equal(ro.last_value, lv), k
        rec = [x.cpu().numpy() for x in (ro.rew, ro.value, ro.last_value, ro._done, ro.env_done, prev)]
        want = gae_ref(*rec, gamma, lam)
        got = [x.cpu().numpy() for x in (ro.adv, ro.ret, ro.mask, ro._done_prev)]
        _assert_exact(got, want, (n, E, one_launch, chains, k))
        if k > 0:                                                                  # the carry: run k's tick 0 sees run k-1's last flags
            carried += int(rec[5].sum())
        ends += int((ro.env_done[1:] != 0).sum())
        prev = ro._done_prev.clone()
    assert ends > 0 and carried > 0                                                # games ended, and agents entered a run already done


def test_rollout_gae_normalised_and_then_sees_the_finished_advantages():
    T, n, E = 32, 1, 384
    actor, critic = _actors(n, seed=8)
    snap = {}

    def then(ro):
        snap["adv"] = ro.adv.clone()                                               # recorded into the same graph, after the GAE launches
        snap["stats"] = ro.adv_stats.clone()
    _, ro = _rollout(n, E, T, False, 1, actor, critic, gae=dict(gamma=0.98, lam=0.9, normalize=True), then=then)
    prev = ro._done_prev.clone()
    for k in range(3):
        ro.run()
        torch.cuda.synchronize()
        assert torch.equal(snap["adv"], ro.adv) and torch.equal(snap["stats"], ro.adv_stats), k
        rec = [x.cpu().numpy() for x in (ro.rew, ro.value, ro.last_value, ro._done, ro.env_done, prev)]
        want = gae_ref(*rec, 0.98, 0.9, normalize=True)
        got = [x.cpu().numpy() for x in (ro.adv, ro.ret, ro.mask, ro._done_prev, ro.adv_stats)]
        _assert_normalised(got, want, k)
        assert want[4][0] > 0
        prev = ro._done_prev.clone()


# ---- a scripted opponent's agents have no decisions

def _assert_stats_exact(got, want, what):
    assert np.array_equal(got[4].view(np.int64), want[4].view(np.int64)), (what, "stats", got[4], want[4])


@pytest.mark.parametrize("normalize", [False, True], ids=["plain", "normalize"])
@pytest.mark.parametrize("T,E,A", [(7, 33, 2), (9, 21, 6), (4, 64, 8), (5, 19, 10)])
def test_gae_with_agents_flagged_off_is_bit_identical_to_the_restatement(T, E, A, normalize):
    """advantage.gae(agents=f) (bsx_gae_agents): each team alone and an irregular pattern, at 2 and 4 columns a lane -- (9, 21, 6) and
    (5, 19, 10) have an odd E: two-column lanes whose columns lie in two games.  adv, ret, mask, the carry and -- against the kernel's own
    merge order restated -- the float64 statistics, to the bit.  Every flag set gives the bits of the call without the argument (bsx_gae)."""
    rng = np.random.default_rng(1000 * T + A)
    case = random_case(rng, T, E, A)
    if normalize:
        case[0][...] += 0.5
    half = A // 2
    flags = (np.array([1] * half + [0] * half, np.uint8), np.array([0] * half + [1] * half, np.uint8),
             np.array([(7 * a + 3) % 5 < 3 for a in range(A)], np.uint8))
    for f in flags:
        got, want = _run(case, 0.99, 0.95, normalize, agents=f), gae_ref(*case, 0.99, 0.95, normalize, agents=f, kernel_order=True)
        _assert_exact(got, want, (T, E, A, f))
        assert (got[0][..., f == 0].view(np.int32) == 0).all() and (got[1][..., f == 0].view(np.int32) == 0).all() and not got[2][..., f == 0].any()
        if normalize:
            _assert_stats_exact(got, want, (T, E, A, f))
            assert got[4][0] == got[2].sum() > 0
    plain = _run(case, 0.99, 0.95, normalize)
    for none in (_run(case, 0.99, 0.95, normalize, agents=np.ones(A, np.uint8)), _run(case, 0.99, 0.95, normalize, agents=np.ones(A, bool))):
        _assert_exact(none, plain, (T, E, A, "no flag"))
        if normalize:
            _assert_stats_exact(none, plain, (T, E, A, "no flag"))
    _assert_exact(plain, gae_ref(*case, 0.99, 0.95, normalize, kernel_order=True), (T, E, A, "plain"))


# (kind, n, one_launch, scripted team, E): PolicyRollout(opponent=instinct.Team(...), gae=dict(..., normalize=True)), T = 8
OPPONENT_ROLLOUTS = [("categorical", 2, False, "blue", 96), ("categorical", 1, True, "red", 160), ("gaussian", 2, False, "blue", 96)]


@pytest.mark.parametrize("kind,n,one_launch,opponent,E", OPPONENT_ROLLOUTS, ids=lambda v: str(v))
def test_rollout_with_a_scripted_opponent_masks_its_rows_and_keeps_them_out_of_the_statistics(kind, n, one_launch, opponent, E):
    """The actor does not play the scripted team: its columns carry mask 0 and adv = ret = +0, the learned columns are the restatement
    (agents=) of the rollout's own records bit for bit -- the normalised advantages and (n, mean, std) included, which are those of
    the learned rows alone."""
    import ppo_learner_util as L
    ro = L.small_rollout(kind, n=n, E=E, one_launch=one_launch, opponent=opponent, normalize=True, runs=1)
    scripted, learned = L.scripted_columns(n, opponent)
    prev = ro._done_prev.clone()
    ro.run()
    torch.cuda.synchronize()
    assert ro.one_launch == one_launch and ro.opponent.team == (0 if opponent == "red" else 1)
    flag = np.zeros(2 * n, np.uint8)
    flag[learned] = 1
    assert not ro.mask[..., scripted].any()
    assert bool((ro.adv[..., scripted].view(torch.int32) == 0).all()) and bool((ro.ret[..., scripted].view(torch.int32) == 0).all())
    rec = [x.cpu().numpy() for x in (ro.rew, ro.value, ro.last_value, ro._done, ro.env_done, prev)]
    want = gae_ref(*rec, 0.99, 0.95, normalize=True, agents=flag, kernel_order=True)
    got = [x.cpu().numpy() for x in (ro.adv, ro.ret, ro.mask, ro._done_prev, ro.adv_stats)]
    assert int(got[2].sum()) > 100 and got[2][..., learned].any(-1).any()
    print(kind, n, opponent, "masked rows", int(got[2].sum()), "stats", got[4], "restated", want[4])
    _assert_exact(got, want, (kind, n, one_launch, opponent))
    assert float(ro.adv_stats[0]) == float(ro.mask.sum())
    _assert_stats_exact(got, want, (kind, n, one_launch, opponent))
