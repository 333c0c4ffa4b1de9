"""CPU-side checks of the prioritised replay ring (csrc/bsx_replay_prio.hip): its entry points are declared, exported and bound, the
node buffer's size against replay.prio_levels, argument validation before any launch (fake addresses only: a call that got through
would return a HIP error on a machine without a GPU), the Python surface, and the numpy reference of tests/prio_util.py itself: at
M = 4097 (three levels) and, before the GPU is held to it there, at 64^3 + 1 and 64^4 + 67 (four and five levels; the level counts
of the four sizes of tests/test_hip_replay_prio_deep.py are written out in DEEP_LEVELS).  No kernel is launched here."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import prio_util as PU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("bsx_replay_prio_bytes", "bsx_replay_prio_rebuild", "bsx_replay_prio_sample", "bsx_replay_prio_weights", "bsx_replay_prio_update",
         "bsx_replay_prio_append")
ARG, ALIGN = -1, -2
A = 4096                      # a 256-byte aligned fake address (never dereferenced)
SIZES = (1, 63, 64, 65, 4096, 4097, 262_144, 262_145, 16_777_283, (1 << 31) - 1)
# the level counts, bottom-up, of the sizes the GPU suite checks at depth (tests/test_hip_replay_prio_deep.py), written out
DEEP_LEVELS = {4096: (64, 1), 262_144: (4096, 64, 1), 262_145: (4097, 65, 2, 1), 16_777_283: (262_146, 4097, 65, 2, 1)}


def _lib():
    from deep_rl_battlespace_amd import _lib
    return _lib


def test_prio_symbols_are_declared_exported_and_bound():
    import deep_rl_battlespace_amd as pkg
    hdr = open(os.path.join(ROOT, "include", "battlespace_hip.h")).read()
    declared = set(re.findall(r"^\s*int\s+(bsx_\w+)\s*\(", hdr, flags=re.M))
    lib = _lib().load()
    for name in NAMES:
        assert name in declared and name in _lib().SIGNATURES and hasattr(lib, name), name
    assert "typedef struct BsxPrioTree" in hdr and [f for f, _ in _lib().BsxPrioTree._fields_] == ["leaves", "nodes", "max_priority", "hyper", "M"]
    assert lib.bsx_abi_version() == 14 and re.search(r"#define BSX_ABI_VERSION 14\b", hdr)       # additive: the ABI version stays
    salt = int(re.search(r"#define BSX_PRIO_SALT (0x[0-9A-Fa-f]+)u", hdr).group(1), 16)
    assert salt == PU.SALT == _lib().PRIO_SALT and salt != 0x5EED5A3C
    assert (_lib().PRIO_FANOUT, _lib().PRIO_ONE) == (PU.FAN, PU.ONE) == (64, 65536)
    assert "PrioritizedReplayBuffer" in pkg.__all__ and pkg.PrioritizedReplayBuffer is pkg.replay.PrioritizedReplayBuffer


@pytest.mark.parametrize("M", SIZES)
def test_node_buffer_bytes_match_prio_levels(M):
    from deep_rl_battlespace_amd.replay import prio_levels
    lv = prio_levels(M)
    assert lv == PU.levels(M) and lv[0] == (0, -(-M // 64)) and lv[-1][1] == 1
    for (o0, c0), (o1, c1) in zip(lv, lv[1:]):
        assert o1 == o0 + c0 and c1 == -(-c0 // 64)
    sz = ctypes.c_size_t()
    assert _lib().load().bsx_replay_prio_bytes(M, ctypes.byref(sz)) == 0 and sz.value == 8 * sum(c for _, c in lv)


@pytest.mark.parametrize("M", sorted(DEEP_LEVELS))
def test_levels_and_node_buffer_bytes_at_four_and_five_levels_are_the_literal_counts(M):
    from deep_rl_battlespace_amd.replay import prio_levels
    counts = DEEP_LEVELS[M]
    offsets = tuple(sum(counts[:k]) for k in range(len(counts)))
    assert tuple(PU.DEEP_SIZES) == tuple(sorted(DEEP_LEVELS)) and (PU.M4, PU.M5) == (262_145, 16_777_283)
    assert PU.levels(M) == prio_levels(M) == list(zip(offsets, counts))
    sz = ctypes.c_size_t()
    assert _lib().load().bsx_replay_prio_bytes(M, ctypes.byref(sz)) == 0 and sz.value == 8 * sum(counts)
    assert {262_145: 8 * 4165, 16_777_283: 8 * 266_311}.get(M, sz.value) == sz.value


def test_node_buffer_bytes_refusals():
    lib, sz = _lib().load(), ctypes.c_size_t()
    for M in (0, -1, 1 << 31):
        assert lib.bsx_replay_prio_bytes(M, ctypes.byref(sz)) == ARG
    assert lib.bsx_replay_prio_bytes(64, None) == ARG
    from deep_rl_battlespace_amd.replay import prio_levels
    for M in (0, 1 << 31):
        with pytest.raises(ValueError):
            prio_levels(M)


def _tree(**kw):
    f = dict(leaves=A, nodes=A, max_priority=A, hyper=A, M=1000)
    f.update(kw)
    return _lib().BsxPrioTree(*(f[k] for k, _ in _lib().BsxPrioTree._fields_))


def _ring(**kw):
    f = dict(obs=A, obs_next=A, act=A, rew=A, done=A, counter=A, M=1000, nA=2, D=8, n_act=4)
    f.update(kw)
    return _lib().BsxReplayRing(*(f[k] for k, _ in _lib().BsxReplayRing._fields_))


# every call's tree: BSX_E_ARG for a missing pointer or M out of range, BSX_E_ALIGN for leaves, nodes, max_priority or hyper off their boundary
TREE_ARG = [dict(leaves=None), dict(nodes=None), dict(max_priority=None), dict(hyper=None), dict(M=0), dict(M=-4), dict(M=1 << 31)]
TREE_ALIGN = [dict(leaves=A + 2), dict(nodes=A + 4), dict(max_priority=A + 2), dict(hyper=A + 8), dict(hyper=A + 4)]


def _run(call, cases):
    for want, kw in cases:
        assert call(**kw) == want, kw


def test_rebuild_rejects_bad_arguments_before_any_launch():
    lib = _lib().load()

    def rebuild(tree=None, no_tree=False):
        return lib.bsx_replay_prio_rebuild(None if no_tree else ctypes.byref(_tree(**(tree or {}))), None)
    _run(rebuild, [(ARG, dict(no_tree=True))] + [(ARG, dict(tree=t)) for t in TREE_ARG] + [(ALIGN, dict(tree=t)) for t in TREE_ALIGN]
         + [(ARG, dict(tree=dict(nodes=A + 4, M=0))), (ARG, dict(tree=dict(hyper=A + 4, leaves=None)))])


def test_update_rejects_bad_arguments_before_any_launch():
    lib = _lib().load()

    def update(tree=None, idx=A, q=A, y=A, B=512, nA=2, no_tree=False):
        return lib.bsx_replay_prio_update(None if no_tree else ctypes.byref(_tree(**(tree or {}))), idx, q, y, B, nA, None)
    cases = [(ARG, dict(no_tree=True))] + [(ARG, dict(tree=t)) for t in TREE_ARG] + [(ARG, {k: None}) for k in ("idx", "q", "y")]
    cases += [(ARG, dict(B=0)), (ARG, dict(B=-1)), (ARG, dict(B=1 << 31)), (ARG, dict(nA=0)), (ARG, dict(nA=17))]
    cases += [(ALIGN, dict(tree=t)) for t in TREE_ALIGN] + [(ALIGN, dict(idx=A + 4)), (ALIGN, dict(q=A + 2)), (ALIGN, dict(y=A + 2))]
    # two rules broken at once: every BSX_E_ARG is found before any BSX_E_ALIGN
    cases += [(ARG, dict(idx=A + 4, B=0)), (ARG, dict(tree=dict(nodes=A + 4), q=None)), (ARG, dict(tree=dict(hyper=A + 4), nA=17)),
              (ARG, dict(q=A + 2, tree=dict(M=0)))]
    _run(update, cases)


def test_append_rejects_bad_arguments_before_any_launch():
    lib = _lib().load()

    def append(tree=None, counter=A, stored=A, rows=64, no_tree=False):
        return lib.bsx_replay_prio_append(None if no_tree else ctypes.byref(_tree(**(tree or {}))), counter, stored, rows, None)
    cases = [(ARG, dict(no_tree=True))] + [(ARG, dict(tree=t)) for t in TREE_ARG]
    cases += [(ARG, dict(counter=None)), (ARG, dict(stored=None)), (ARG, dict(rows=0)), (ARG, dict(rows=1 << 31))]
    cases += [(ALIGN, dict(tree=t)) for t in TREE_ALIGN] + [(ALIGN, dict(counter=A + 4)), (ALIGN, dict(stored=A + 4))]
    cases += [(ARG, dict(counter=A + 4, rows=0)), (ARG, dict(tree=dict(leaves=A + 2), stored=None)), (ARG, dict(stored=A + 4, tree=dict(M=0)))]
    _run(append, cases)


def test_weights_rejects_bad_arguments_before_any_launch():
    lib = _lib().load()

    def weights(tree=None, idx=A, B=512, nA=2, w=A, ws=A, no_tree=False):
        return lib.bsx_replay_prio_weights(None if no_tree else ctypes.byref(_tree(**(tree or {}))), idx, B, nA, w, ws, None)
    cases = [(ARG, dict(no_tree=True))] + [(ARG, dict(tree=t)) for t in TREE_ARG] + [(ARG, {k: None}) for k in ("idx", "w", "ws")]
    cases += [(ARG, dict(B=0)), (ARG, dict(B=1 << 31)), (ARG, dict(nA=0)), (ARG, dict(nA=17))]
    cases += [(ALIGN, dict(tree=t)) for t in TREE_ALIGN] + [(ALIGN, dict(idx=A + 4)), (ALIGN, dict(w=A + 2)), (ALIGN, dict(ws=A + 2))]
    cases += [(ARG, dict(idx=A + 4, B=0)), (ARG, dict(ws=A + 2, w=None)), (ARG, dict(tree=dict(hyper=A + 8), nA=0))]
    _run(weights, cases)


def test_sample_rejects_bad_arguments_before_any_launch():
    lib = _lib().load()

    def sample(ring=None, tree=None, B=512, seq_base=A, idx=A, obs=A, obs_next=A, act=A, rew=A, done=A, w=A, ws=A, no_ring=False, no_tree=False):
        r = None if no_ring else ctypes.byref(_ring(**(ring or {})))
        t = None if no_tree else ctypes.byref(_tree(**(tree or {})))
        return lib.bsx_replay_prio_sample(r, t, B, 0, 0, seq_base, idx, obs, obs_next, act, rew, done, w, ws, None)
    cases = [(ARG, dict(no_ring=True)), (ARG, dict(no_tree=True)), (ARG, dict(B=0)), (ARG, dict(B=-1)), (ARG, dict(B=1 << 31))]
    cases += [(ARG, dict(tree=t)) for t in TREE_ARG] + [(ARG, dict(tree=dict(M=999)))]         # the tree must be the ring's
    cases += [(ARG, {k: None}) for k in ("idx", "obs", "obs_next", "act", "rew", "done", "w", "ws")]
    cases += [(ARG, dict(ring=kw)) for kw in (dict(counter=None), dict(M=0), dict(M=1 << 31), dict(nA=17), dict(D=51), dict(n_act=1))]
    cases += [(ALIGN, dict(tree=t)) for t in TREE_ALIGN] + [(ALIGN, {k: A + 2}) for k in ("obs", "obs_next", "act", "rew", "w", "ws")]
    cases += [(ALIGN, dict(idx=A + 4)), (ALIGN, dict(seq_base=A + 4)), (ALIGN, dict(ring=dict(counter=A + 4))), (ALIGN, dict(ring=dict(act=A + 2)))]
    cases += [(ARG, dict(idx=A + 4, B=0)), (ARG, dict(tree=dict(hyper=A + 4), obs=None)), (ARG, dict(tree=dict(nodes=A + 4), ring=dict(D=0))),
              (ARG, dict(ws=A + 2, tree=dict(max_priority=None))), (ARG, dict(ring=dict(counter=A + 4), tree=dict(M=0)))]
    _run(sample, cases)


def test_prioritized_replay_buffer_has_the_base_constructor_plus_four_keywords():
    import torch
    from deep_rl_battlespace_amd.replay import DeviceReplayBuffer, PrioritizedReplayBuffer
    base = list(inspect.signature(DeviceReplayBuffer.__init__).parameters.values())
    mine = list(inspect.signature(PrioritizedReplayBuffer.__init__).parameters.values())
    assert [(p.name, p.default) for p in mine[:-4]] == [(p.name, p.default) for p in base]
    assert [(p.name, p.default) for p in mine[-4:]] == [("alpha", 0.6), ("beta", 0.4), ("eps", 1e-6), ("delta_max", 32.0)]
    for name in ("append_rollout", "store_rollout", "store_transition", "sample", "is_ready", "update_priorities", "set_alpha", "set_beta",
                 "rebuild_tree"):
        assert callable(getattr(PrioritizedReplayBuffer, name)), name
    assert list(inspect.signature(PrioritizedReplayBuffer.update_priorities).parameters) == ["self", "q", "y", "idx"]
    buf = PrioritizedReplayBuffer(4097, 4, ["plane0", "plane1"], 8, 16, 4, device="cpu")
    assert buf.priorities.shape == (4097,) and buf.priorities.dtype == torch.int32 and buf._leaves.shape == (4160,) and not buf._leaves.any()
    assert buf.tree.shape == (65 + 2 + 1,) and buf.tree.dtype == torch.int64
    assert int(buf.max_priority) == 65536 and buf.weights.shape == (4, 2) and buf.last_idx.shape == (4,)
    assert buf.prio_hyper.tolist() == [float(np.float32(x)) for x in (0.6, 0.4, 1e-6, 32.0)]
    # the counter cannot be moved from outside: the tree would no longer describe the ring
    assert buf.mem_cntr == 0 and not buf.is_ready()
    for value in (5, 0, -1):
        with pytest.raises(ValueError, match="priority tree"):
            buf.mem_cntr = value
    assert buf.mem_cntr == 0
    for kw in (dict(alpha=-0.1), dict(beta=-1.0), dict(eps=-1e-3), dict(delta_max=0.0), dict(alpha=float("nan"))):
        with pytest.raises(ValueError):
            PrioritizedReplayBuffer(16, 4, ["plane0"], 8, 8, 4, device="cpu", **kw)
    with pytest.raises(ValueError):
        PrioritizedReplayBuffer(16, 4, ["plane0"], 8, 8, 5, device="cpu")


# ------------------------------------------------------------------------------------------------ the reference itself
def test_reference_draws_follow_the_priorities_and_never_name_a_zero_leaf():
    """200 000 reference draws over leaves [1, 0, 3, 2^31, 1] at a fixed seed: the zero leaf never appears and every row's frequency lies
    within 5 binomial standard deviations of p / total.  A condition on the reference (prio_util.draw_rows), not on the kernel."""
    leaves, n = np.array([1, 0, 3, 1 << 31, 1], np.int64), 200_000
    rows = PU.draw_rows(leaves, seed=11, seq=0, B=n)
    counts, total = np.bincount(rows, minlength=5), int(leaves.sum())
    assert counts.sum() == n and counts[1] == 0
    for r, p in enumerate(leaves):
        share = p / total
        assert abs(counts[r] - n * share) <= 5.0 * np.sqrt(n * share * (1.0 - share)), (r, counts[r], n * share)
    assert not PU.draw_rows(np.zeros(5, np.int64), 11, 0, 7).any()              # an empty ring: row 0


def test_reference_u_is_the_high_word_of_the_128_bit_product():
    r = PU.draw_r(3, 5, 4)
    assert all(0 <= x < 1 << 64 for x in r) and len(set(r)) == 4 and r != PU.draw_r(3, 6, 4) and r != PU.draw_r(4, 5, 4)
    total = (1 << 62) - 1
    u = PU.draw_u(3, 5, 4, total)
    assert all(int(a) == (b * total) >> 64 and 0 <= int(a) < total for a, b in zip(u, r))
    # the sampler's words under the prioritised salt, not the uniform sampler's
    import philox_util as P
    w = P.philox4x32_10(np.arange(4), 0, 5, 0, 3, PU.SALT)
    assert [(int(h) << 32) | int(l) for l, h in zip(w[0], w[1])] == r
    assert int(P.sampler_words(3, 5, np.arange(4, dtype=np.uint64))[0][0]) != r[0] & 0xFFFFFFFF


def test_reference_descent_is_searchsorted():
    """The level-by-level descent a kernel makes agrees with cumsum + searchsorted on 10 000 draws at M = 4097 (three levels)."""
    leaves = PU.random_leaves(4097)
    assert (leaves == 0).sum() > 1000 and leaves.max() == 1 << 31 and leaves[leaves > 0].min() == 1
    lv = PU.tree_levels(leaves)
    assert [len(x) for x in lv] == [65, 2, 1] and int(lv[-1][0]) == int(leaves.sum()) and len(PU.node_buffer(leaves)) == 68
    u = PU.draw_u(2, 0, 10_000, int(leaves.sum()))
    rows = PU.rows_of(leaves, u)
    assert np.array_equal(PU.descend(leaves, u), rows) and (leaves[rows] > 0).all() and len(np.unique(rows)) > 50
    edge = np.array([0, int(leaves.sum()) - 1], np.int64)                      # the first and the last unit of mass
    assert np.array_equal(PU.descend(leaves, edge), PU.rows_of(leaves, edge))
    assert PU.rows_of(leaves, edge)[0] == np.flatnonzero(leaves)[0] and PU.rows_of(leaves, edge)[1] == np.flatnonzero(leaves)[-1]


def test_reference_leaf_patterns_and_edge_rows():
    assert PU.edge_rows(4096).tolist() == [0, 63, 64, 4094, 4095]
    assert PU.edge_rows(262_144).tolist() == [0, 63, 64, 4095, 4096, 262_142, 262_143]
    assert PU.edge_rows(PU.M4).tolist() == [0, 63, 64, 4095, 4096, 262_143, 262_144]
    top = 1 << 24
    assert PU.edge_rows(PU.M5).tolist() == [0, 63, 64, 4095, 4096, 262_143, 262_144, top - 1, top, top + 1, top + 3, PU.M5 - 2, PU.M5 - 1]
    assert int(np.float32(top + 1)) == top and int(np.float32(top + 3)) == top + 4                 # neither survives a float32
    p = PU.needle_leaves(70, [0, 69], 5)
    assert p.dtype == np.int64 and p.sum() == 10 and p[0] == p[69] == 5
    for M in (5, 64, PU.M4):
        h = PU.heavy_leaves(M)
        assert h.dtype == np.int64 and set(np.unique(h)) <= {PU.P_MAX - 1, PU.P_MAX} and int(h.sum()) % 2 == 1
    assert PU.pattern_leaves(PU.M4, "needles") is PU.pattern_leaves(PU.M4, "needles") and not PU.pattern_leaves(PU.M4, "needles").flags.writeable


@pytest.mark.parametrize("pattern", PU.PATTERNS)
@pytest.mark.parametrize("M", [PU.M4, PU.M5])
def test_reference_descent_is_searchsorted_at_four_and_five_levels(M, pattern):
    """10 000 draws per leaf pattern: the descent through four and five levels names the rows of cumsum + searchsorted, the needles on
    the node boundaries are all found (the odd rows above 2^24 among them) and a total past 2^53 keeps its lowest bit."""
    leaves = PU.pattern_leaves(M, pattern)
    lv, total = PU.tree_levels(leaves), int(leaves.sum())
    assert tuple(len(x) for x in lv) == DEEP_LEVELS[M] and int(lv[-1][0]) == total and len(PU.node_buffer(leaves)) == sum(DEEP_LEVELS[M])
    u = PU.draw_u(2, 0, 10_000, total)
    rows = PU.rows_of(leaves, u)
    assert np.array_equal(PU.descend(leaves, u), rows) and (leaves[rows] > 0).all()
    edge = np.array([0, total - 1], np.int64)
    assert np.array_equal(PU.descend(leaves, edge), PU.rows_of(leaves, edge))
    assert PU.rows_of(leaves, edge).tolist() == [np.flatnonzero(leaves)[0], np.flatnonzero(leaves)[-1]]
    if pattern == "needles":
        assert set(rows) == set(PU.edge_rows(M))
    if pattern == "heavy":
        assert total % 2 == 1 and (M != PU.M5 or (total > 1 << 53 and int(float(total)) != total))
    if pattern == "random":
        assert len(np.unique(rows >> 12)) >= 64 and len(np.unique(rows)) > 5000            # draws from all over the ring


def test_reference_append_update_priorities_and_weights():
    leaves = np.array([5, 0, 7, 0, 9], np.int64)
    assert PU.append_range(leaves, 7, 3, 100).tolist() == [100, 100, 7, 0, 100]        # rows (7 - 3 + j) mod 5 = 4, 0, 1: across the wrap
    assert PU.append_range(leaves, 12, 9, 3).tolist() == [3] * 5 and PU.append_range(leaves, 4, 0, 3).tolist() == leaves.tolist()
    assert PU.update_max(leaves, np.array([2, 2, 0]), np.array([4, 6, 1])).tolist() == [1, 0, 6, 0, 9]
    hyper = np.array([0.6, 0.4, 1e-6, 32.0], np.float32)
    q = np.array([[0.0, 1.0], [np.nan, 0.0], [100.0, 0.0], [0.0, 0.0]], np.float32)
    y = np.zeros((4, 2), np.float32)
    ref, yard = PU.priority_ref(q, y, hyper), PU.priority_yard(q, y, hyper)
    top = (32.0 + float(np.float32(1e-6))) ** float(np.float32(0.6)) * 65536
    assert abs(ref[0] - (1.0 + float(np.float32(1e-6))) ** float(np.float32(0.6)) * 65536) < 1e-6 and ref[1] == ref[2] == top
    assert np.abs(yard - ref).max() <= 0.5 + 1e-6 * top and (yard == np.rint(yard)).all()
    assert (PU.priority_ref(q, y, np.array([0.0, 0.4, 1e-6, 32.0], np.float32)) == 65536).all()      # alpha = 0: uniform
    assert (PU.priority_yard(q, y, np.array([0.0, 0.4, 1e-6, 32.0], np.float32)) == 65536).all()
    p = np.array([4, 1 << 31, 0, 4, 64])
    w = PU.weights_ref(p, 0.5)
    assert w[0] == w[3] == 1.0 and w[2] == 0.0 and abs(w[4] - 0.25) < 1e-12 and np.abs(PU.weights_yard(p, 0.5) - w).max() < 1e-7
    assert (PU.weights_ref(p, 0.0)[p > 0] == 1.0).all() and not PU.weights_ref(np.zeros(3), 0.4).any()
