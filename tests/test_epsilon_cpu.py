"""CPU-side checks of epsilon-greedy exploration (BsxActorNoise.epsilon / .explored, bsx_epsilon_advance, PolicyRollout(epsilon=),
rollout.EpsilonSchedule): the header and the binding agree on the grown struct and the new entry point; every refusal comes before any
launch, with its code (fake addresses only: no call here reaches a kernel); the host restatement of the rule (tests/epsilon_util.py),
which the GPU is held to bit for bit, explores at the asked rate with uniform actions from a stream of its own; the linear schedule's
restatement; PolicyRollout and FusedActor validate their arguments on a stub env."""
import ctypes
import os
import re
import types
from fractions import Fraction

import numpy as np
import pytest
import torch

import epsilon_util as EU
import philox_util as PU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG, ALIGN = -1, -2
P, M = 4096, 4096 + 8          # a 256-byte aligned fake address and one aligned to 8 bytes only (neither is dereferenced)


def _lib():
    from deep_rl_battlespace_amd import _lib as L
    return L


def _noise(L, **fields):
    nz = L.BsxActorNoise()
    for k, v in fields.items():
        setattr(nz, k, v)
    return ctypes.byref(nz)


def test_header_and_binding_agree_on_the_grown_struct_and_the_schedule_entry():
    L = _lib()
    hdr = open(os.path.join(ROOT, "include", "battlespace_hip.h")).read()
    body = re.search(r"typedef struct BsxActorNoise \{(.*?)\} BsxActorNoise;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [f for decl in body.split(";") for f in re.findall(r"\b(\w+)\s*(?:,|$)", decl.strip())]
    names = [f for f, _ in L.BsxActorNoise._fields_]
    assert fields == names and names[-3:] == ["value", "epsilon", "explored"]          # appended at the END, after `value`

    class Before(ctypes.Structure):
        _fields_ = L.BsxActorNoise._fields_[:-2]
    assert ctypes.sizeof(Before) == 96 and ctypes.sizeof(L.BsxActorNoise) == ctypes.sizeof(Before) + 16
    assert L.BsxActorNoise.epsilon.offset == 96 and L.BsxActorNoise.explored.offset == 104
    nz = L.BsxActorNoise(0.1, 0.0, 0.15, 0.2, 0.0, None, None, None, 0, 0, 0.0, None, None, None, None)     # a positional use of before
    assert nz.epsilon is None and nz.explored is None
    assert re.search(r"^int\s+bsx_epsilon_advance\s*\(", hdr, flags=re.M) and "bsx_epsilon_advance" in L.SIGNATURES
    assert hasattr(L.load(), "bsx_epsilon_advance")
    assert L.load().bsx_abi_version() == 14 == L.ABI_VERSION                            # additive: the ABI version stays
    src = open(os.path.join(ROOT, "deep-rl-battlespace_amd", "csrc", "bsx_actor_core.h")).read()
    assert re.search(r"EPS_SALT = 0x20000000u", src) and L.EPS_SALT == EU.EPS_SALT == 0x20000000
    assert EU.EPS_SALT not in (PU.SALT_OU, PU.SALT_GAUSS_WITH_OU, PU.SALT_CATEGORICAL, 0xC0000000)


def test_actor_forward_refuses_epsilon_combinations_before_any_launch():
    L = _lib(); lib = L.load()

    def fwd(nz, scores=P, off=0):
        return lib.bsx_actor_forward(P, P, scores, 4, 1, 0, nz, 0, 0, None, off, None)

    cases = [(ARG, dict(epsilon=P, gaussian_std=0.1)), (ARG, dict(epsilon=P, ou_scale=0.5, ou_state=P)), (ARG, dict(epsilon=P, ou_scale=0.5)),
             (ARG, dict(epsilon=P, ou_scale=0.5, ou_state=M)), (ARG, dict(epsilon=P, sample_mode=1, temperature=1.0)),
             (ARG, dict(epsilon=P, sample_mode=2, temperature=1.0)), (ARG, dict(explored=P)), (ARG, dict(explored=P, gaussian_std=0.1)),
             (ALIGN, dict(epsilon=P + 2)), (ALIGN, dict(epsilon=P + 2, explored=P)), (ALIGN, dict(epsilon=P + 1)),
             (ALIGN, dict(epsilon=P, u_inject=M)),                                    # injected uniforms are taken with epsilon, and checked
             (ARG, dict(epsilon=P + 2, gaussian_std=0.1)), (ARG, dict(explored=P, epsilon=None, z_inject=M))]
    for want, kw in cases:
        assert fwd(_noise(L, **kw)) == want, kw
    assert fwd(_noise(L, epsilon=P, explored=P + 1), off=-1) == ARG                   # (every epsilon check passed: the last refusal of the call)
    assert fwd(_noise(L, epsilon=P), scores=M) == ALIGN
    # the Gaussian head excludes it
    head = ctypes.byref(L.BsxGaussianHead(P, None))
    assert lib.bsx_actor_forward_gaussian(P, P, P, 4, 1, 0, _noise(L, epsilon=P), head, 0, 0, None, 0, None) == ARG
    assert lib.bsx_actor_forward_gaussian(P, P, P, 4, 1, 0, _noise(L, explored=P), head, 0, 0, None, 0, None) == ARG
    # sample_mode keeps its two values
    assert fwd(_noise(L, sample_mode=2, temperature=1.0)) == ARG


def test_rollouts_refuse_epsilon_combinations_before_any_launch():
    L = _lib(); lib = L.load()
    rw = ctypes.byref(L.BsxRewards(100, 10, -1, -5, -20))

    def disc(nz, n=1, state=P):
        return lib.bsx_rollout_discrete(state, 4, n, 8, P, 0, -1, P, P, P, P, None, None, None, rw, 0, nz, 0, 0, None, 0, 0, None)

    def cont(nz):
        return lib.bsx_rollout_continuous(P, 4, 1, 8, P, 0, -1, 0, P, P, P, P, None, None, None, rw, 0, nz, 0, 0, None, 0, 0, None)

    def gauss(nz):
        return lib.bsx_rollout_continuous_gaussian(P, 4, 1, 8, P, 0, -1, 0, P, P, P, P, None, None, None, rw, 0, nz,
                                                   ctypes.byref(L.BsxGaussianHead(P, None)), 0, 0, None, 0, 0, None)

    cases = [(ARG, dict(epsilon=P, gaussian_std=0.1)), (ARG, dict(epsilon=P, ou_scale=0.5, ou_state=P)), (ARG, dict(epsilon=P, ou_scale=0.5, ou_state=M)),
             (ARG, dict(epsilon=P, sample_mode=1, temperature=1.0)), (ARG, dict(epsilon=P, sample_mode=2, temperature=1.0)),
             (ARG, dict(explored=P)), (ARG, dict(epsilon=P, u_inject=P)), (ARG, dict(epsilon=P, explored=P, z_inject=P)),
             (ALIGN, dict(epsilon=P + 2)), (ALIGN, dict(epsilon=P + 2, explored=P)), (ARG, dict(epsilon=P + 2, gaussian_std=0.1))]
    for want, kw in cases:
        for n in (1, 2, 3, 4):
            assert disc(_noise(L, **kw), n=n) == want, (kw, n)
    assert disc(_noise(L, epsilon=P), state=M) == ALIGN and disc(_noise(L, epsilon=P, gaussian_std=0.1), state=M) == ALIGN   # the state's checks come first
    for kw in (dict(epsilon=P), dict(epsilon=P, explored=P), dict(explored=P), dict(epsilon=P + 2)):       # a continuous env, with or without the head
        assert cont(_noise(L, **kw)) == ARG, kw
        assert gauss(_noise(L, **kw)) == ARG, kw
    assert disc(_noise(L, sample_mode=2, temperature=1.0)) == ARG


def test_epsilon_advance_refuses_before_any_launch():
    lib = _lib().load()

    def adv(eps=P, A=2, count=P, by=1, start=1.0, end=0.1, steps=10, kind=0):
        return lib.bsx_epsilon_advance(eps, A, count, by, start, end, steps, kind, None)

    nan = float("nan")
    cases = [(ARG, dict(A=0)), (ARG, dict(A=-3)), (ARG, dict(steps=0)), (ARG, dict(steps=-1)), (ARG, dict(kind=2)), (ARG, dict(kind=-1)),
             (ARG, dict(start=1.5)), (ARG, dict(start=-0.1)), (ARG, dict(end=1.0001)), (ARG, dict(end=-1e-9)), (ARG, dict(start=nan)),
             (ARG, dict(end=nan)), (ARG, dict(eps=None)), (ARG, dict(count=None)), (ALIGN, dict(eps=P + 2)), (ALIGN, dict(count=P + 4)),
             (ARG, dict(A=0, eps=P + 2)), (ARG, dict(kind=2, count=P + 4))]
    for want, kw in cases:
        assert adv(**kw) == want, kw


SEED, ROWS, SEQS, RATE = 20261021, 65536, 8, 0.25


def test_the_restated_rule_explores_at_the_asked_rate_with_uniform_actions_from_its_own_stream():
    """The only statistical test: the GPU is held to this restatement bit for bit.  65 536 rows x 8 sequence numbers at epsilon = 0.25."""
    grow = np.arange(ROWS, dtype=np.uint64)
    ux, act = zip(*(EU.draws(SEED, seq, grow) for seq in range(SEQS)))
    ux, act = np.stack(ux), np.stack(act)
    assert ux.dtype == np.float32 and float(ux.min()) > 0.0 and float(ux.max()) < 1.0 and act.min() == 0 and act.max() == 3
    flags = ux < np.float32(RATE)
    N = flags.size
    share = flags.mean()
    print("explored share", share, "of", N)
    assert abs(share - RATE) <= 5.0 * np.sqrt(RATE * (1.0 - RATE) / N)
    k = int(flags.sum())
    for a in range(4):
        sa = float((act[flags] == a).mean())
        print("action", a, "share among explored", sa)
        assert abs(sa - 0.25) <= 5.0 * np.sqrt(0.25 * 0.75 / k)
    # int(u.y * 4.0f) is the top two bits of the 23-bit code
    w = np.stack([PU.actor_words(SEED, seq, grow, EU.EPS_SALT)[1] for seq in range(SEQS)])
    assert np.array_equal(act, (w >> np.uint32(30)).astype(np.int32))
    # a stream of its own: not the categorical head's uniforms
    other = np.stack([PU.uniforms4(SEED, seq, grow, PU.SALT_CATEGORICAL)[..., 0] for seq in range(SEQS)]) < np.float32(RATE)
    assert not np.array_equal(flags, other) and abs(float((flags & other).mean()) - RATE * RATE) < 0.01       # and independent of them


def test_the_restated_rule_on_rows_edge_rates_and_injected_uniforms():
    rng = np.random.default_rng(3)
    E, A = 37, 4
    greedy = np.tanh(rng.standard_normal((E, A, 4))).astype(np.float32)
    eps = np.array([0.0, 1.0, 0.3, np.nan], np.float32)
    out, ex = EU.apply(greedy, eps, SEED, 5, env_offset=11)
    assert not ex[:, 0].any() and ex[:, 1].all() and not ex[:, 3].any() and 0 < ex[:, 2].sum() < E
    assert np.array_equal(out[ex == 0], greedy[ex == 0])
    assert (np.abs(out[ex == 1]) == 1.0).all() and ((out[ex == 1] == 1.0).sum(-1) == 1).all()
    grow = (11 + np.arange(E, dtype=np.uint64))[:, None] * np.uint64(A) + np.arange(A, dtype=np.uint64)
    assert np.array_equal(out[ex == 1].argmax(-1), EU.draws(SEED, 5, grow)[1][ex == 1])
    u = rng.random((E, A, 4)).astype(np.float32)
    out_u, ex_u = EU.apply(greedy, np.full(A, 0.5, np.float32), SEED, 5, u=u)
    assert np.array_equal(ex_u, (u[..., 0] < 0.5).astype(np.uint8)) and np.array_equal(out_u[ex_u == 1].argmax(-1), (u[..., 1] * 4).astype(int)[ex_u == 1])
    assert np.array_equal(EU.apply(greedy, np.full(A, -1.0, np.float32), SEED, 5)[0], greedy)                  # epsilon <= 0: greedy, bit for bit


@pytest.mark.parametrize("start,end,steps", [(1.0, 0.1, 20), (0.9, 0.05, 7), (0.25, 0.75, 1000003), (1.0, 0.0, 1)])
def test_the_linear_schedule_restated(start, end, steps):
    counts = [0, 1, steps - 1, steps, steps + 5]
    got = [EU.schedule(c, start, end, steps) for c in counts]
    assert all(g.dtype == np.float32 for g in got)
    assert got[0] == np.float32(start) and got[3] == np.float32(end) and got[4] == np.float32(end)
    for c, g in zip(counts, got):                    # the exact rational value, within one float32 ulp
        exact = Fraction(end) + (Fraction(start) - Fraction(end)) * max(Fraction(0), 1 - Fraction(c, steps))
        assert abs(Fraction(float(g)) - exact) <= Fraction(float(np.spacing(np.float32(max(start, end))))), (c, g)
        assert g == np.float32(end + (start - end) * max(0.0, 1.0 - c / steps))
    d, inc = np.sign(end - start), [float(g) for _, g in sorted(zip(counts, got))]
    assert all(d * (b - a) >= 0 for a, b in zip(inc, inc[1:]))
    assert EU.schedule(5, 1.0, 0.1, 10, "exponential") == np.float32(0.1 + 0.9 * np.exp(-0.5))


def _stub_env(n=1, E=8, continuous=False):
    return types.SimpleNamespace(_compat=False, rng="philox", continuous_actions=continuous, n_agents=n, n_envs=E, _A=2 * n,
                                 obs_size=3 * n + 2, device=torch.device("cpu"), env_offset=0)


def test_policy_rollout_validates_epsilon():
    from deep_rl_battlespace_amd.rollout import EpsilonSchedule, PolicyRollout, StackedActor
    env, actor = _stub_env(), StackedActor(2, 5, 4)
    with pytest.raises(ValueError, match="fused"):
        PolicyRollout(env, actor, 4, epsilon=0.1, fused=False, chains=1)
    with pytest.raises(ValueError, match="discrete"):
        PolicyRollout(_stub_env(continuous=True), StackedActor(2, 5, 3), 4, epsilon=0.1, chains=1)
    with pytest.raises(ValueError, match="excludes"):
        PolicyRollout(env, actor, 4, epsilon=0.1, sample="categorical", chains=1)
    with pytest.raises(ValueError, match="excludes"):
        PolicyRollout(env, actor, 4, epsilon=0.1, noise_std=0.1, chains=1)
    with pytest.raises(ValueError, match="excludes"):
        PolicyRollout(env, actor, 4, epsilon=0.1, ou_scale=0.2, chains=1)
    with pytest.raises(ValueError, match="fused"):
        PolicyRollout(env, actor, 4, epsilon=EpsilonSchedule(1.0, 0.1, 100), fused=False, chains=1)
    for bad in (torch.zeros(3), torch.zeros(2, dtype=torch.float64), torch.zeros((2, 1)), torch.zeros(4)[::2]):
        with pytest.raises(ValueError, match="epsilon"):
            PolicyRollout(env, actor, 4, epsilon=bad, chains=1)
    mine = torch.tensor([0.5, 0.25])
    ro = PolicyRollout(env, actor, 4, epsilon=mine, chains=1)
    assert ro.epsilon is mine and ro.explored.dtype == torch.bool and tuple(ro.explored.shape) == (4, 8, 2) and not ro.explored.any()
    for form in (dict(chains=1), dict(one_launch=True), dict(chains=2)):
        ro = PolicyRollout(_stub_env(n=2), StackedActor(4, 8, 4), 4, epsilon=0.3, **form)
        assert ro.epsilon.dtype == torch.float32 and ro.epsilon.tolist() == [np.float32(0.3)] * 4
    ro = PolicyRollout(env, actor, 4, chains=1)
    assert ro.epsilon is None and ro.explored is None
    for kw in (dict(start=1.5, end=0.1, steps=10), dict(start=1.0, end=-0.1, steps=10), dict(start=1.0, end=0.1, steps=0),
               dict(start=1.0, end=0.1, steps=10, kind="cosine"), dict(start=1.0, end=0.1, steps=10, unit="games")):
        with pytest.raises(ValueError):
            EpsilonSchedule(**kw)


def test_fused_actor_noise_struct_validates_epsilon():
    from deep_rl_battlespace_amd.rollout import FusedActor, StackedActor
    fa = FusedActor(StackedActor(2, 5, 4), 1)
    ev, ex, u = torch.zeros(2), torch.zeros((6, 2), dtype=torch.uint8), torch.zeros((6, 2, 4))
    nz = fa.noise_struct(6, epsilon=dict(value=ev, explored=ex, u=u))
    assert nz.epsilon == ev.data_ptr() and nz.explored == ex.data_ptr() and nz.u_inject == u.data_ptr() and nz.sample_mode == 0
    nz = fa.noise_struct(6, epsilon=dict(value=ev, explored=torch.zeros((3, 6, 2), dtype=torch.uint8)))      # a [T, E, A] record
    assert nz.explored is not None and nz.u_inject is None
    assert fa.noise_struct(6) is None
    for bad in (dict(value=torch.zeros(3)), dict(value=torch.zeros(2, dtype=torch.float64)), dict(value=0.1), dict(value=torch.zeros(4)[::2]),
                dict(value=ev, explored=torch.zeros((6, 2), dtype=torch.bool)), dict(value=ev, explored=torch.zeros((5, 2), dtype=torch.uint8)),
                dict(value=ev, u=torch.zeros((6, 2, 3))), dict(value=ev, u=torch.zeros((6, 2, 4), dtype=torch.float64))):
        with pytest.raises(ValueError, match="epsilon"):
            fa.noise_struct(6, epsilon=bad)
    for kw in (dict(noise_std=0.1), dict(sample=dict(temperature=1.0)), dict(ou=dict(scale=0.1, state=torch.zeros((6, 2, 4))))):
        with pytest.raises(ValueError, match="excludes"):
            fa.noise_struct(6, epsilon=dict(value=ev), **kw)
    with pytest.raises(ValueError, match="discrete"):
        FusedActor(StackedActor(2, 5, 3), 1).noise_struct(6, epsilon=dict(value=ev))
