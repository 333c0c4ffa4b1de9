"""What the GPU tests of the prioritised replay ring share (tests/test_hip_replay_prio.py, tests/test_hip_replay_prio_deep.py): rings of a
given shape, random rows and TD pairs to feed them, and the comparison of a ring's tree with the numpy reference of tests/prio_util.py.
The package is imported inside the functions that build a ring: importing this module needs neither the native library nor a GPU."""
import numpy as np
import torch

import prio_util as PU

RING_FIELDS = ("actor_states", "actor_new_states", "action_mem", "rew_mem", "done_mem")
OBS = 8


def buf(M, B, nA=1, k=4, seed=0, D_=OBS, **kw):
    from deep_rl_battlespace_amd.replay import PrioritizedReplayBuffer
    return PrioritizedReplayBuffer(M, B, list(range(nA)), D_, D_ * nA, k, device="cuda", seed=seed, **kw)


def plain(M, B, nA=1, k=4, seed=0, D_=OBS):
    from deep_rl_battlespace_amd.replay import DeviceReplayBuffer
    return DeviceReplayBuffer(M, B, list(range(nA)), D_, D_ * nA, k, device="cuda", seed=seed)


def rows(R, nA, k, seed, D_=OBS):
    g = torch.Generator(device="cuda"); g.manual_seed(seed)
    rnd = lambda *s: torch.randn(s, generator=g, device="cuda")                         # noqa: E731
    return rnd(R, nA, D_), rnd(R, nA, k), rnd(R, nA), rnd(R, nA, D_), torch.rand((R, nA), generator=g, device="cuda") < 0.3


def set_leaves(ring, p):
    ring.priorities.copy_(PU.as_leaves(p))
    ring.rebuild_tree()


def leaves(ring):
    return PU.unsigned(ring.priorities)


def assert_tree_exact(ring, what=""):
    """Every level is the exact sum of the leaves read back; the pad leaves are 0.  -> the leaves read back (one read-back per check)."""
    torch.cuda.synchronize()
    got = leaves(ring)
    assert np.array_equal(ring.tree.cpu().numpy(), PU.node_buffer(got)), what
    assert not ring._leaves[ring.mem_size:].any(), what
    return got


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def td_pairs(B, nA, seed):
    """q, y float32 [B, nA]: errors from 1e-4 to 1e3 (some above delta_max = 32), a NaN in about one row in eight."""
    g = np.random.default_rng(seed)
    y = g.standard_normal((B, nA)).astype(np.float32)
    q = (y + g.choice([-1.0, 1.0], (B, nA)) * 10.0 ** g.uniform(-4.0, 3.0, (B, nA))).astype(np.float32)
    q[g.random((B, nA)) < 0.125 / nA] = np.nan
    return q, y


def assert_same_ring(ring, twin, what):
    for f in RING_FIELDS:
        assert torch.equal(bits(getattr(ring, f)), bits(getattr(twin, f))), (what, f)
    assert ring.mem_cntr == twin.mem_cntr, what
