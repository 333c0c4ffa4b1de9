"""The prioritised replay ring (csrc/bsx_replay_prio.hip, replay.PrioritizedReplayBuffer) on the MI355X at four and five levels, where
tests/test_hip_replay_prio.py stops at three (M = 4097: bsx_prio_repair_kernel runs for level 0 only, whose children are leaves).  The
sizes are prio_util.DEEP_SIZES:
  4096 = 64^2 and 262 144 = 64^3   exact: (64, 1) and (4096, 64, 1) nodes; a level of exactly 64 nodes still belongs to the tail workgroup
  M4 = 64^3 + 1                    (4097, 65, 2, 1): repair launches for levels 0 and 1, the last node of every level has one child
  M5 = 64^4 + 67                   (262 146, 4097, 65, 2, 1): repair launches for levels 0, 1 and 2; rows 2^24 + 1 and 2^24 + 3 exist, and
                                   a ring of leaves near 2^31 has a total past 2^53
Every quantity is an integer with one right value, so everything but the weights is compared bit for bit with tests/prio_util.py: every
level after a rebuild, an update (BY_IDX and WHOLE at inner levels, see UPDATES) and an append (BY_RANGE at inner levels, across the
wrap and under three nodes of a level), the rows drawn through four and five dependent loads, and the rows gathered, which carry their
own index in their bits (prio_util.stamp_ring).  The rings are narrow (one agent, one observation word, three actions: 25 bytes a row);
the M5 leaf patterns are built once per process (prio_util.pattern_leaves)."""
import numpy as np
import pytest
import torch

import guard_util as G
import prio_ring_util as R
import prio_util as PU
import yardstick_util as Y

pytestmark = pytest.mark.gpu

M4, M5 = PU.M4, PU.M5
NA, OBS, K = 1, 1, 3


def _ring(M, B, seed=0):
    return R.buf(M, B, NA, K, seed=seed, D_=OBS)


def _report_peak(M, what):
    if M == M5:
        print(f"{what} at M = {M}: peak torch.cuda.max_memory_allocated() {torch.cuda.max_memory_allocated() / 2 ** 30:.3f} GiB")


def _fresh_peak():
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()


# ------------------------------------------------------------------------------------------------ rebuild, draw, gather, weights
@pytest.mark.parametrize("pattern", PU.PATTERNS)
@pytest.mark.parametrize("M", PU.DEEP_SIZES)
def test_every_level_the_rows_drawn_their_stamps_and_the_weights(M, pattern):
    B, seed = 512, 9
    _fresh_peak()
    p = PU.pattern_leaves(M, pattern)
    drawn = [PU.draw_rows(p, seed, call, B) for call in range(4)]
    if pattern == "needles":                                                            # from the reference alone: every needle is drawn
        assert set(np.concatenate(drawn[:3])) == set(PU.edge_rows(M)) and (M != M5 or {(1 << 24) + 1, (1 << 24) + 3} <= set(drawn[0]))
    buf = _ring(M, B, seed=seed)
    PU.stamp_ring(buf)
    R.set_leaves(buf, p)
    buf.rebuild_tree()                     # once more, over the nodes the first rebuild wrote (not the zeros of a new ring): no change
    torch.cuda.synchronize()
    tree = buf.tree.cpu().numpy()
    for k, ((off, cnt), want) in enumerate(zip(PU.levels(M), PU.tree_levels(p))):
        assert np.array_equal(tree[off:off + cnt], want), f"level {k}"
    assert len(tree) == sum(c for _, c in PU.levels(M)) and int(tree[-1]) == int(p.sum())
    assert np.array_equal(R.leaves(buf), p) and not buf._leaves[M:].any()
    beta = float(buf.prio_hyper[1])
    for call in range(3):
        buf.sample()
        torch.cuda.synchronize()
        want = drawn[call]
        assert np.array_equal(buf.last_idx.cpu().numpy(), want), call                   # every b, exactly
        assert (p[want] > 0).all() and int(buf._draws) == call + 1
        for field in (buf._b_obs, buf._b_obs_, buf._b_act):
            assert np.array_equal(PU.stamps(field), want), call                         # the rows gathered say which rows they are
        w = buf.weights.cpu().numpy()
        assert w.shape == (B, NA)
        ref, yard = PU.weights_ref(p[want], beta), PU.weights_yard(p[want], beta)
        assert ref.max() == 1.0 and w.max() == 1.0
        _, bad = Y.check_tensors([("weights", w[:, 0].astype(np.float64), ref, yard, Y.FACTORS)], f"M{M} {pattern} call {call}", unit="w")
        assert not bad
    buf.set_beta(0.0)
    buf.sample()
    torch.cuda.synchronize()
    assert np.array_equal(buf.last_idx.cpu().numpy(), drawn[3]) and bool((buf.weights == 1.0).all())      # beta = 0: exactly 1
    _report_peak(M, f"draw ({pattern})")


# ------------------------------------------------------------------------------------------------ update
# (M, B, the repair mode of every level below the tail workgroup's, bottom-up): a level of more nodes than the batch has rows is repaired
# BY_IDX, one wave per row named; any other WHOLE, one wave per node.  Both run at an inner level (1 or 2) at both depths.
UPDATES = [(M4, 33, ("BY_IDX", "BY_IDX")), (M4, 512, ("BY_IDX", "WHOLE")),
           (M5, 33, ("BY_IDX", "BY_IDX", "BY_IDX")), (M5, 512, ("BY_IDX", "BY_IDX", "WHOLE")), (M5, 4100, ("BY_IDX", "WHOLE", "WHOLE"))]


def _repair_modes(M, B):
    """What bsx_replay_prio_update does per level: the levels before the first of at most 64 nodes get a launch each."""
    counts = [c for _, c in PU.levels(M)]
    first = next(k for k, c in enumerate(counts) if c <= PU.FAN)
    return tuple("BY_IDX" if c > B else "WHOLE" for c in counts[:first])


def _update_rows(M, B):
    """B rows of [0, M): random ones, then every edge row, two rows under one level-1 node but under different level-0 nodes (two waves
    write one node), and the first of the two once more (a row named twice)."""
    g = np.random.default_rng(50 + M + B)
    rows = g.integers(0, M, B)
    a = 5 * 4096 + 3
    forced = np.concatenate([PU.edge_rows(M), [a, a + 7 * 64, a]])
    assert a >> 12 == (a + 7 * 64) >> 12 and a >> 6 != (a + 7 * 64) >> 6 and len(forced) <= B
    rows[B - len(forced):] = forced
    return rows


@pytest.mark.parametrize("M,B,modes", UPDATES, ids=[f"M{m}-B{b}" for m, b, _ in UPDATES])
def test_update_repairs_the_inner_levels_by_row_and_whole(M, B, modes):
    assert _repair_modes(M, B) == modes
    _fresh_peak()
    buf, one = _ring(M, B), _ring(64, 1)
    old = PU.pattern_leaves(M, "random")
    R.set_leaves(buf, old)
    rows = _update_rows(M, B)
    idx = torch.from_numpy(rows).cuda()
    q, y = R.td_pairs(B, NA, 60 + M + B)
    assert np.isnan(q).any() and (np.abs(q - y) > 32.0).any() and (np.abs(q - y) < 1.0).any()
    tq, ty = torch.from_numpy(q).cuda(), torch.from_numpy(y).cuda()
    buf.update_priorities(tq, ty, idx)
    # what the kernel writes per occurrence: the same inputs one row per call, occurrence b on row b % 64 of a 64-row ring of its own
    slot = torch.arange(64, device="cuda")
    occ = torch.zeros(B, dtype=torch.int32, device="cuda")
    for b in range(B):
        one.update_priorities(tq[b:b + 1], ty[b:b + 1], slot[b % 64:b % 64 + 1])
        if b % 64 == 63 or b == B - 1:
            occ[b - b % 64:b + 1].copy_(one.priorities[:b % 64 + 1])
    torch.cuda.synchronize()
    occ = PU.unsigned(occ)
    assert (occ >= 1).all() and (occ <= PU.P_MAX).all() and len(np.unique(occ)) > B // 4
    got = R.assert_tree_exact(buf)                                                       # the whole node buffer; the pad leaves are 0
    assert np.array_equal(got, PU.update_max(old, rows, occ))                            # the maximum per named row; the others untouched
    assert len(np.unique(rows)) < B and PU.unsigned(buf.max_priority)[0] == max(PU.ONE, int(occ.max()))
    R.assert_tree_exact(one)
    _report_peak(M, f"update (B = {B})")


# ------------------------------------------------------------------------------------------------ append
def _check_append(buf, want, stored, maxp, what):
    got = R.assert_tree_exact(buf, what)
    assert np.array_equal(got, want), what
    assert int(buf._stored) == stored and PU.unsigned(buf.max_priority)[0] == maxp, what


def test_append_at_four_levels_across_the_wrap_past_the_ring_and_under_three_level_1_nodes():
    """The sequence of test_hip_replay_prio.py's append test at M4 -- the second step writes rows M - 2, M - 1, 0, 1, 2: the one-child last
    node of every level and node 0, three nodes where the host's bound of waves is three --, then two steps placed by the running counter:
    one inside a single level-1 node, one of 4098 rows from the last leaf of a level-1 node (three level-1 nodes, bound four).  Each
    against DeviceReplayBuffer for the ring and prio_util.append_range for the leaves."""
    M = M4
    buf, twin = _ring(M, 4), R.plain(M, 4, NA, K, D_=OBS)
    want, counter = np.zeros(M, np.int64), 0

    def step(n, maxp, what):
        nonlocal want, counter
        buf.max_priority.copy_(PU.as_leaves([maxp]))                                     # raised first: the rows must carry this value
        rows = R.rows(n, NA, K, 10 * M + counter % 1000, D_=OBS)
        for b in (buf, twin):
            b._put(*rows)
        counter += n
        want = PU.append_range(want, counter, n, maxp)
        _check_append(buf, want, n, maxp, what)
        R.assert_same_ring(buf, twin, what)

    for n, maxp in ((M - 2, 65536), (5, 200_001), (M + 70, 1 << 31), (1, 77), (2 * M, 65_537)):
        step(n, maxp, f"{n} rows")
        assert n != M - 2 or ((want[:M - 2] > 0).all() and not want[M - 2:].any())       # rows never stored are still 0
    pos = counter % M
    inside = min(1000, ((pos >> 12) + 1 << 12) - pos)
    assert inside > 128 and pos >> 12 == (pos + inside - 1) >> 12 and pos >> 6 != (pos + inside - 1) >> 6
    step(inside, 300_000, "inside one level-1 node")
    step((4095 - counter % M) % 4096 or 4096, 70_000, "up to the last leaf of a level-1 node")
    pos = counter % M
    assert pos % 4096 == 4095 and pos + 4098 < M and ((pos + 4097) >> 12) - (pos >> 12) == 2
    step(4098, 99_999, "4098 rows under three level-1 nodes")
    assert sorted(np.unique(want)) == [65_537, 70_000, 99_999, 300_000]


def test_append_at_five_levels_across_the_wrap_and_under_three_level_2_nodes():
    """M5, no twin ring and no step longer than the ring: a fill of M - 2 rows, three rows across the wrap (M - 2, M - 1, 0), one row, then
    up to the last leaf of a level-2 node and 262 146 rows from there (three level-2 nodes, where the host's bound of waves is four), then
    up to row 64^4 - 1 and 69 rows from there: across the wrap under four level-0 nodes and three of levels 1 and 2 -- at every launched
    level exactly the host's bound of waves (M - 2 and M - 1 share a level-0 node: the three-row step stays one below it)."""
    M = M5
    _fresh_peak()
    buf = _ring(M, 4)
    z = lambda *s: torch.zeros(s, device="cuda")                                         # noqa: E731
    src = (z(M, NA, OBS), z(M, NA, K), z(M, NA), z(M, NA, OBS), torch.zeros((M, NA), dtype=torch.bool, device="cuda"))
    want, counter = np.zeros(M, np.int64), 0
    for n, maxp, what in ((M - 2, 65536, "fill"), (3, 200_001, "across the wrap"), (1, 1 << 31, "one row"),
                          (262_141, 77, "up to the last leaf of a level-2 node"), (262_146, 65_537, "under three level-2 nodes"),
                          (64 ** 4 - 1 - 524_289, 123_456, "up to row 64^4 - 1"), (69, 999_999, "69 rows across the wrap, the bound at every level")):
        pos = counter % M
        if n == 69:
            assert pos == 64 ** 4 - 1 and pos + n == M + 1
            assert all(((M - 1) >> s) - (pos >> s) + 2 == (n >> s) + 3 for s in (6, 12, 18))
        if n == 262_146:
            assert pos % 262_144 == 262_143 and ((pos + n - 1) >> 18) - (pos >> 18) == 2 and pos + n < M
        buf.max_priority.copy_(PU.as_leaves([maxp]))
        buf._put(*(t[:n] for t in src))
        counter += n
        want = PU.append_range(want, counter, n, maxp)
        _check_append(buf, want, n, maxp, what)
        assert what != "fill" or ((want[:M - 2] > 0).all() and not want[M - 2:].any())   # rows never stored are still 0
    assert buf.mem_cntr == counter == 2 * M + 1
    _report_peak(M, "append")


# ------------------------------------------------------------------------------------------------ guards
def test_no_stray_writes_at_four_levels():
    """M4, B = 33: leaves, nodes, weights, last_idx, max_priority and the weights' workspace inside guard slabs."""
    from deep_rl_battlespace_amd import _lib
    M, B = M4, 33
    buf = _ring(M, B, seed=2)
    mk = G.Buffers(guarded=True)
    buf._leaves = mk("leaves", buf._leaves.shape, torch.int32)
    buf.priorities = buf._leaves[:M]
    buf.tree = mk("nodes", buf.tree.shape, torch.int64)
    buf.weights = mk("weights", (B, NA), torch.float32)
    buf.last_idx = mk("last_idx", (B,), torch.int64)
    buf.max_priority = mk("max_priority", (1,), torch.int32, init=65536)
    buf._drawn = mk("drawn", (B,), torch.int32)
    buf._tree = _lib.BsxPrioTree(buf._leaves.data_ptr(), buf.tree.data_ptr(), buf.max_priority.data_ptr(), buf.prio_hyper.data_ptr(), M)
    buf.rebuild_tree()
    for step, n in enumerate((M - 3, 70, M + 5000, 1)):                                   # up to the wrap, across it, past the ring, one row
        buf._put(*R.rows(n, NA, K, step, D_=OBS))
        R.assert_tree_exact(buf, step)
    p = PU.random_leaves(M, seed=4)
    p[M - 1] = 1 << 31                                                                   # the last row: the one child of every level's last node
    R.set_leaves(buf, p)
    for call in range(3):
        buf.sample()
        q, y = (torch.from_numpy(a).cuda() for a in R.td_pairs(B, NA, call))
        buf.update_priorities(q, y)
        R.assert_tree_exact(buf, call)
    buf.last_idx.copy_(torch.arange(M - B, M, device="cuda"))                            # the rows at the very end of the ring
    buf.update_priorities(q, y)
    buf.sample()
    R.assert_tree_exact(buf, "end")
    assert mk.stray() == []


# ------------------------------------------------------------------------------------------------ capture
def test_a_captured_sample_and_update_at_four_levels_replays_the_eager_calls():
    M, B, seed = M4, 512, 5
    buf, eager = _ring(M, B, seed=seed), _ring(M, B, seed=seed)
    p = PU.pattern_leaves(M, "random")
    q, y = (torch.from_numpy(a).cuda() for a in R.td_pairs(B, NA, 3))
    buf.sample(); buf.update_priorities(q, y)                                             # warm-up outside the capture, then as constructed
    buf._draws.zero_(); buf.max_priority.fill_(PU.ONE)
    for b in (buf, eager):
        R.set_leaves(b, p)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        buf.sample()
        buf.update_priorities(q, y)
    assert int(buf._draws) == 0 and np.array_equal(R.assert_tree_exact(buf, "captured, not run"), p)
    leaves, draws = p, []
    for call in range(3):
        graph.replay()
        eager.sample(); eager.update_priorities(q, y)
        torch.cuda.synchronize()
        assert torch.equal(buf.last_idx, eager.last_idx) and torch.equal(buf.weights.view(torch.int32), eager.weights.view(torch.int32)), call
        assert torch.equal(buf._leaves, eager._leaves) and torch.equal(buf.tree, eager.tree), call
        assert torch.equal(buf.max_priority, eager.max_priority), call
        rows = buf.last_idx.cpu().numpy()
        assert np.array_equal(rows, PU.draw_rows(leaves, seed, call, B)), call             # drawn from the tree the replay before left
        before, leaves = leaves, R.assert_tree_exact(buf, call)
        assert not np.array_equal(before, leaves)
        draws.append(rows)
    assert not np.array_equal(draws[0], draws[1]) and not np.array_equal(draws[1], draws[2]) and int(buf._draws) == 3
