"""The device replay ring (csrc/bsx_replay.hip, replay.DeviceReplayBuffer) on the MI355X: what it stores is what the torch ring
(ReplayBuffer) stores, bit for bit, row by row and counter for counter; what it samples is the base's tuple for the drawn indices; it
records into a HIP graph together with the rollout; and it writes nothing outside its arrays."""
import ctypes
import os

import numpy as np
import pytest
import torch

from guard_util import guards_intact as _guards_intact, slab as _slab

pytestmark = pytest.mark.gpu

RING_FIELDS = ("actor_states", "actor_new_states", "action_mem", "rew_mem", "done_mem")


def _env(**kw):
    import deep_rl_battlespace_amd as bsx
    return bsx.parallel_env(**kw)


def _buffers(M, B, agents, D, n_act, seed=0):
    from deep_rl_battlespace_amd.replay import DeviceReplayBuffer, ReplayBuffer
    nA = len(agents)
    return (ReplayBuffer(M, B, agents, D, D * nA, n_act, device="cuda"),
            DeviceReplayBuffer(M, B, agents, D, D * nA, n_act, device="cuda", seed=seed))


def _assert_rings_equal(ref, dev, what):
    for f in RING_FIELDS:
        assert torch.equal(getattr(ref, f), getattr(dev, f)), (what, f)
    assert ref.mem_cntr == dev.mem_cntr, (what, ref.mem_cntr, dev.mem_cntr)


def _assert_batches_equal(a, b, what):
    assert len(a) == len(b) == 7
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and x.dtype == y.dtype and torch.equal(x, y), (what, i)


def _rollout(n, E, T, cont, one_launch, seed):
    from deep_rl_battlespace_amd import instinct
    from deep_rl_battlespace_amd.rollout import PolicyRollout, StackedActor
    env = _env(n_agents=n, n_envs=E, seed=seed, auto_reset=True, continuous_actions=cont); env.reset()
    torch.manual_seed(seed)
    actor = StackedActor(2 * n, 3 * n + 2, 3 if cont else 4, device="cuda")
    with torch.no_grad():
        actor.w3.mul_(100.0)
    # the scripted blue team makes games decisive early, so game ends (and the re-spawn rows, which are not transitions) fall in
    ro = PolicyRollout(env, actor, T, noise_std=0.2, one_launch=one_launch, opponent=instinct.Team(env.possible_blue, env.possible_red, env))
    ro.start()
    return env, ro


# (n, E, T, team, continuous, one_launch, M): red / blue columns, discrete / continuous (3 actions from 4-wide score rows), the
# one-launch and the graph form (5v5: graph only), a ring that wraps inside a rollout, a ring smaller than one rollout's kept rows
CASES = [(1, 64, 16, "red", False, True, 40000),
         (1, 96, 16, "blue", True, True, 1500),
         (2, 128, 16, "blue", False, False, 3000),
         (4, 64, 12, "red", True, True, 5000),
         (5, 40, 12, "red", False, False, 2000),
         (2, 256, 16, "red", False, True, 1000)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}v{c[0]}-{c[3]}-{'cont' if c[4] else 'disc'}-{'one' if c[5] else 'graph'}-M{c[6]}")
def test_append_equals_store_rollout_bit_for_bit(case):
    n, E, T, team, cont, one_launch, M = case
    env, ro = _rollout(n, E, T, cont, one_launch, seed=5 + n)
    cols = range(n) if team == "red" else range(n, 2 * n)
    agents = env.possible_red if team == "red" else env.possible_blue
    ref, dev = _buffers(M, 64, agents, env.obs_size, 3 if cont else 4)
    ro.capture()
    dropped, over, wrapped = 0, False, False
    for rep in range(12):
        ro.run()
        old = ref.mem_cntr
        want = ref.store_rollout(ro, cols)
        word = dev.append_rollout(ro, cols)
        assert int(word.item()) == want, rep
        _assert_rings_equal(ref, dev, rep)
        dropped += int((ro.env_done[:T] != 0).sum())
        over |= want > M
        wrapped |= want < M and old % M + want > M
    assert dropped > 0                                       # rows of finished games were skipped
    if M < 40000:
        assert ref.mem_cntr > M
    if M == 1000:
        assert over                                          # R > M: only the newest M rows are written
    elif M < 40000:
        assert wrapped                                       # the ring wrapped inside one rollout
    # a rollout with no kept rows leaves the ring and the counter as they are
    snap = [getattr(dev, f).clone() for f in RING_FIELDS]
    cnt = dev.mem_cntr
    ro.env_done[:T].fill_(1)
    assert ref.store_rollout(ro, cols) == 0 and dev.store_rollout(ro, cols) == 0
    assert dev.mem_cntr == cnt and all(torch.equal(s, getattr(dev, f)) for s, f in zip(snap, RING_FIELDS))
    _assert_rings_equal(ref, dev, "empty")


def test_g10_reference_buffer_through_the_device_counter():
    """g10 (maddpg/buffer.py run unmodified; as trace_util.check_replay_against_reference drives the base) through
    DeviceReplayBuffer.store_transition: ring snapshots, mem_cntr, is_ready and sample(idx=...) are the reference's."""
    from deep_rl_battlespace_amd.replay import DeviceReplayBuffer
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g10_replay_buffer.npz"))
    M, B, obs_size, n_act, nA = (int(v) for v in g["cfg"])
    agents = [f"plane{i}" for i in range(nA)]
    buf = DeviceReplayBuffer(M, B, agents, obs_size, obs_size * nA, n_act, device="cuda", seed=1)
    S = g["in/states"].shape[0]
    checked = 0
    for k in range(S):
        d = lambda key: {a: g["in/" + key][k, i] for i, a in enumerate(agents)}     # noqa: E731
        buf.store_transition(d("states"), d("actions"), d("rewards"), d("states_"), d("dones"))
        tag = f"after{k + 1}"
        if tag + "/mem_cntr" not in g.files:
            continue
        checked += 1
        assert buf.mem_cntr == int(g[tag + "/mem_cntr"]) and buf.is_ready() == bool(g[tag + "/is_ready"])
        np.testing.assert_array_equal(buf.state_mem.cpu().numpy(), g[tag + "/state_mem"].astype(np.float32))
        np.testing.assert_array_equal(buf.new_state_mem.cpu().numpy(), g[tag + "/new_state_mem"].astype(np.float32))
        np.testing.assert_array_equal(buf.rew_mem.cpu().numpy(), g[tag + "/rew_mem"].astype(np.float32))
        np.testing.assert_array_equal(buf.done_mem.cpu().numpy(), g[tag + "/done_mem"])
        for name, mine in (("actor_states", buf.actor_states), ("actor_new_states", buf.actor_new_states), ("action_mem", buf.action_mem)):
            np.testing.assert_array_equal(mine.transpose(0, 1).cpu().numpy(), g[f"{tag}/{name}"].astype(np.float32))
        if tag + "/idx" in g.files:
            res = buf.sample(idx=g[tag + "/idx"])
            for name, v in zip(("actor_states", "states", "actions", "rewards", "actor_new_states", "states_", "dones"), res):
                ref = g[f"{tag}/sample/{name}"]
                assert tuple(v.shape) == ref.shape, name
                np.testing.assert_array_equal(v.cpu().numpy(), ref.astype(np.float32) if ref.dtype != bool else ref, err_msg=name)
    assert checked >= 3 and buf.mem_cntr == S


@pytest.mark.parametrize("one_launch,n", [(True, 1), (False, 2)])
def test_rollout_store_and_sample_as_one_graph(one_launch, n):
    """PolicyRollout.capture(then=...): one replay = T ticks + the append + a learner batch, no host in the graph.  Each replay equals an
    eager twin -- env + rollout, ReplayBuffer.store_rollout, sample(idx=last_idx) -- ring, counter and batch."""
    E, T, M, B = 64, 16, 3000, 256
    env, ro = _rollout(n, E, T, False, one_launch, seed=21)
    twin_env, tw = _rollout(n, E, T, False, one_launch, seed=21)
    ref, dev = _buffers(M, B, env.possible_red, env.obs_size, 4, seed=3)
    out = {}
    ro.capture(then=lambda: out.update(stored=dev.append_rollout(ro, range(n)), batch=dev.sample()))
    prev = None
    for rep in range(5):
        ro.run()
        tw.run()
        torch.cuda.synchronize()
        assert torch.equal(ro.obs, tw.obs) and torch.equal(ro.scores, tw.scores) and torch.equal(ro.env_done, tw.env_done), rep
        want = ref.store_rollout(tw, range(n))
        assert int(out["stored"].item()) == want, rep
        _assert_rings_equal(ref, dev, rep)
        idx = dev.last_idx.clone()
        assert int(idx.max()) < min(dev.mem_cntr, M) and int(idx.min()) >= 0
        _assert_batches_equal(out["batch"], ref.sample(idx=idx), rep)
        assert prev is None or not torch.equal(prev, idx)           # every replay draws afresh
        prev = idx


def test_sampler_range_uniformity_determinism_and_tuple():
    M, B, agents, D = 1000, 4096, ["plane0", "plane1"], 8
    ref, dev = _buffers(M, B, agents, D, 4, seed=11)
    # an empty ring: every index is 0, and row 0 is zeros
    res = dev.sample()
    assert int(dev.last_idx.abs().max()) == 0 and all(float(t.float().abs().max()) == 0.0 for t in res)
    g = torch.Generator(device="cuda")
    for buf in (ref, dev):                                            # the same random ring contents in both
        g.manual_seed(0)
        buf.actor_states.copy_(torch.randn(buf.actor_states.shape, generator=g, device="cuda"))
        buf.actor_new_states.copy_(torch.randn(buf.actor_new_states.shape, generator=g, device="cuda"))
        buf.action_mem.copy_(torch.rand(buf.action_mem.shape, generator=g, device="cuda"))
        buf.rew_mem.copy_(torch.randn(buf.rew_mem.shape, generator=g, device="cuda"))
        buf.done_mem.copy_(torch.rand(buf.done_mem.shape, generator=g, device="cuda") < 0.3)
    # a partly filled ring: indices below the counter
    dev.mem_cntr = ref.mem_cntr = 300
    for _ in range(4):
        res = dev.sample()
        idx = dev.last_idx.clone()
        assert int(idx.min()) >= 0 and int(idx.max()) < 300
        _assert_batches_equal(res, ref.sample(idx=idx), "partial")
    # a full ring (counter beyond M): uniform over [0, M) -- chi-square over 16 x 4096 draws, 999 degrees of freedom
    dev.mem_cntr = ref.mem_cntr = 5 * M + 17
    counts = torch.zeros(M, dtype=torch.int64, device="cuda")
    seen = []
    for _ in range(16):
        res = dev.sample()
        idx = dev.last_idx.clone()
        assert int(idx.min()) >= 0 and int(idx.max()) < M
        _assert_batches_equal(res, ref.sample(idx=idx), "full")
        counts += torch.bincount(idx, minlength=M)
        assert all(not torch.equal(idx, s) for s in seen)            # consecutive calls draw afresh
        seen.append(idx)
    exp = 16 * B / M
    chi2 = float(((counts.double() - exp) ** 2 / exp).sum())
    assert 999 - 6 * (2 * 999) ** 0.5 < chi2 < 999 + 6 * (2 * 999) ** 0.5, chi2
    # the same seed draws the same indices, another seed others
    fresh = [_buffers(M, B, agents, D, 4, seed=s)[1] for s in (11, 11, 12)]
    draws = [[], [], []]
    for buf, out in zip(fresh, draws):
        buf.mem_cntr = 5 * M + 17
        for _ in range(3):
            buf.sample()
            out.append(buf.last_idx.clone())
    for k in range(3):
        assert torch.equal(draws[0][k], draws[1][k]) and not torch.equal(draws[0][k], draws[2][k]), k
    # a captured sample() draws afresh on every replay: the same sequence as eager calls
    _, cap = _buffers(M, B, agents, D, 4, seed=11)
    cap.mem_cntr = 5 * M + 17
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap.sample()
    for k in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(cap.last_idx, draws[0][k]), k


def test_no_stray_writes_at_a_ragged_size():
    """The ring, the workspace and the sample outputs sit inside guard slabs; appends of a ragged number of rows (with skipped rows, a
    wrap, and one larger than the ring) and a ragged batch leave every guard element as it was -- and store what ReplayBuffer stores."""
    from deep_rl_battlespace_amd import _lib
    from deep_rl_battlespace_amd.replay import ReplayBuffer
    lib = _lib.load()
    M, nA, D, k, B = 777, 3, 11, 3, 300
    slabs = {}

    def mk(name, n, dtype, fill):
        slabs[name] = (*_slab(n, dtype, fill), fill, n)
        return slabs[name][1]
    r_obs, r_obs_ = mk("obs", M * nA * D, torch.float32, 7.0), mk("obs_", M * nA * D, torch.float32, 7.0)
    r_act, r_rew = mk("act", M * nA * k, torch.float32, 7.0), mk("rew", M * nA, torch.float32, 7.0)
    r_done, r_cnt = mk("done", M * nA, torch.uint8, 0xAB), mk("cnt", 1, torch.int64, -77)
    for t in (r_obs, r_obs_, r_act, r_rew, r_done, r_cnt):
        t.zero_()
    ring = _lib.BsxReplayRing(r_obs.data_ptr(), r_obs_.data_ptr(), r_act.data_ptr(), r_rew.data_ptr(), r_done.data_ptr(), r_cnt.data_ptr(),
                              M, nA, D, k)
    ref = ReplayBuffer(M, B, ["a", "b", "c"], D, D * nA, k, device="cuda")
    stored = mk("stored", 1, torch.int64, -77)
    ws = mk("ws", 2 + (3001 + 255) // 256, torch.int64, -77)
    g = torch.Generator(device="cuda"); g.manual_seed(4)
    for rows in (1001, 613, 1001, 3001, 5):
        obs = torch.randn((rows, nA, D), generator=g, device="cuda")
        obs_ = torch.randn((rows, nA, D), generator=g, device="cuda")
        act = torch.rand((rows, nA, 4), generator=g, device="cuda")                  # 4-wide source rows under a 3-action ring
        rew = torch.randn((rows, nA), generator=g, device="cuda")
        done = (torch.rand((rows, nA), generator=g, device="cuda") < 0.2).to(torch.uint8)
        skip = (torch.rand((rows,), generator=g, device="cuda") < 0.3).to(torch.uint8)
        src = _lib.BsxReplaySource(obs.data_ptr(), nA * D, D, obs_.data_ptr(), nA * D, D, act.data_ptr(), nA * 4, 4, rew.data_ptr(), nA, 1,
                                   done.data_ptr(), nA, 1, skip.data_ptr(), 1)
        _lib.check(lib.bsx_replay_append(ctypes.byref(ring), ctypes.byref(src), rows, ws.data_ptr(), stored.data_ptr(),
                                         torch.cuda.current_stream().cuda_stream), "append")
        keep = (skip == 0).nonzero().squeeze(1)
        ref._put(obs[keep], act[keep][..., :k], rew[keep], obs_[keep], done[keep].bool())
        torch.cuda.synchronize()
        assert int(stored.item()) == keep.numel() and int(r_cnt.item()) == ref.mem_cntr, rows
        assert torch.equal(r_obs.view(M, nA, D), ref.actor_states) and torch.equal(r_obs_.view(M, nA, D), ref.actor_new_states)
        assert torch.equal(r_act.view(M, nA, k), ref.action_mem) and torch.equal(r_rew.view(M, nA), ref.rew_mem)
        assert torch.equal(r_done.view(M, nA), ref.done_mem.to(torch.uint8))
    assert ref.mem_cntr > 2 * M
    o, o_ = mk("s_obs", B * nA * D, torch.float32, 7.0), mk("s_obs_", B * nA * D, torch.float32, 7.0)
    a, r = mk("s_act", B * nA * k, torch.float32, 7.0), mk("s_rew", B * nA, torch.float32, 7.0)
    d, idx = mk("s_done", B * nA, torch.uint8, 0xAB), mk("s_idx", B, torch.int64, -77)
    for seq in range(3):
        _lib.check(lib.bsx_replay_sample(ctypes.byref(ring), B, 5, seq, None, idx.data_ptr(), o.data_ptr(), o_.data_ptr(), a.data_ptr(),
                                         r.data_ptr(), d.data_ptr(), torch.cuda.current_stream().cuda_stream), "sample")
        torch.cuda.synchronize()
        want = ref.sample(idx=idx.clone())
        assert torch.equal(o.view(B, nA, D), want[0].transpose(0, 1)) and torch.equal(o_.view(B, nA, D), want[4].transpose(0, 1))
        assert torch.equal(a.view(B, nA, k), want[2].transpose(0, 1)) and torch.equal(r.view(B, nA), want[3])
        assert torch.equal(d.view(B, nA), want[6].to(torch.uint8))
    for name, (slab, _, fill, n) in slabs.items():
        assert _guards_intact(slab, fill, n), name


def test_full_size_1v1_three_rollouts():
    """65 536 games of 1v1, T = 32, the reference's ring of 1 000 000 rows: three rollouts appended, equal to store_rollout."""
    n, E, T, M = 1, 65536, 32, 1_000_000
    env, ro = _rollout(n, E, T, False, True, seed=3)
    ref, dev = _buffers(M, 512, env.possible_red, env.obs_size, 4)
    ro.capture()
    total = 0
    for rep in range(3):
        ro.run()
        want = ref.store_rollout(ro, range(n))
        assert int(dev.append_rollout(ro, range(n)).item()) == want, rep
        _assert_rings_equal(ref, dev, rep)
        total += want
    assert total > M                                              # the third rollout wrapped the ring
    _assert_batches_equal(dev.sample(), ref.sample(idx=dev.last_idx.clone()), "full size")
