"""The keyed row permutation without a GPU: its numpy restatement (tests/shuffle_util.py) is a bijection at every size class, is pinned
to literal values so that it cannot drift together with the kernel, follows the documented key layout, and shuffles like a uniform
permutation by three deterministic statistics; the two C entry points are declared, bound and refuse what the header documents before
any launch; PPOLearner's shuffle arguments are checked before anything touches a device."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

import shuffle_util as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 2, 3, 5, 7, 768, 2304, 2 ** 16, 2 ** 16 + 1, 2 ** 21)


@pytest.mark.parametrize("N", SIZES)
def test_the_restatement_is_a_bijection(N):
    p = S.perm(N, 41, 7)
    assert p.dtype == np.int64 and p.shape == (N,)
    seen = np.zeros(N, dtype=np.int64)
    np.add.at(seen, p, 1)
    assert bool((seen == 1).all())
    assert S.half_bits(N) == {1: 1, 2: 1, 3: 1, 5: 2, 7: 2, 768: 5, 2304: 6, 2 ** 16: 8, 2 ** 16 + 1: 9, 2 ** 21: 11}[N]
    assert N <= 1 << (2 * S.half_bits(N)) and (N < 3 or 1 << (2 * S.half_bits(N)) < 4 * N)


def test_sixteen_values_are_pinned_and_positions_are_independent():
    want = [160, 652, 351, 464, 723, 476, 444, 529, 89, 829, 424, 304, 359, 10, 324, 264]
    assert S.perm_at(1000, 41, 7, np.arange(16)).tolist() == want
    assert S.perm(1000, 41, 7)[:16].tolist() == want
    assert S.perm_at(1000, 41, 7, [[15, 0], [3, 3]]).tolist() == [[264, 160], [464, 464]]
    # the widest domain (b = 16: x reaches 2^32 - 1) is evaluated per position, far from the whole range
    N = 2 ** 31 - 1
    ends = S.perm_at(N, 41, 7, np.concatenate([np.arange(4096), np.arange(N - 4096, N)]))
    assert ends.min() >= 0 and ends.max() < N and np.unique(ends).size == 8192 and ends.max() > 2 ** 30
    # the longest cycle walk the issue's prototype met: 42 passes at N = 2^16 + 1, where the domain is 4 N
    assert int(S.evaluations(2 ** 16 + 1, 41, 7, np.arange(2 ** 16 + 1)).max()) == 42


def test_the_key_layout_one_change_at_a_time():
    base = S.perm(1000, 41, 7)
    for seed, seq in ((42, 7), (41, 8), (41 + (1 << 32), 7), (41, 7 + (1 << 32))):
        assert not np.array_equal(S.perm(1000, seed, seq), base), (seed, seq)
    import philox_util as P
    lo = [int(x) for x in P.philox4x32_10(0, 0, 7, 0, 41, S.SHUFFLE_SALT)]
    hi = [int(x) for x in P.philox4x32_10(1, 0, 7, 0, 41, S.SHUFFLE_SALT)]
    assert S.round_keys(41, 7) == lo + hi
    assert S.SHUFFLE_SALT not in (P.ACTOR_KEY_XOR, P.SAMPLER_KEY_XOR, P.OPPONENT_CTR_XOR)
    src = open(os.path.join(ROOT, "deep-rl-battlespace_amd", "csrc", "bsx_shuffle.hip")).read()
    assert int(re.search(r"SHUFFLE_SALT = (0x[0-9A-Fa-f]+)u", src).group(1), 16) == S.SHUFFLE_SALT
    assert int(re.search(r"constexpr int ROUNDS = (\d+);", src).group(1)) == S.ROUNDS


def test_the_permutation_shuffles_like_a_uniform_one():
    """N = 768 rows in M = 4 minibatches, seed 41, seq 0 .. 511: how often each row lands in minibatch 0 (binomial(512, 1/4) for a
    uniform permutation), how often source neighbours stay neighbours (about 2 per permutation), and that no permutation repeats."""
    N, M, K = 768, 4, 512
    perms = np.stack([S.perm(N, 41, seq) for seq in range(K)])
    count = np.zeros(N)
    for p in perms:
        count[p[:N // M]] += 1
    mean, var = K / M, K * (1 / M) * (1 - 1 / M)
    chi = float(((count - mean) ** 2 / var).mean())
    worst = float(np.abs(count - mean).max() / np.sqrt(var))
    adjacent = float(np.mean([(np.abs(np.diff(p)) == 1).sum() for p in perms]))
    print(f"chi-square per row {chi:.4f}, worst row {worst:.3f} sd, adjacent pairs per permutation {adjacent:.4f}")
    assert 0.85 <= chi <= 1.15
    assert worst <= 5.0
    assert 1.5 <= adjacent <= 2.5
    assert len({p.tobytes() for p in perms}) == K


def test_both_entry_points_are_declared_exported_and_bound():
    from deep_rl_battlespace_amd import _lib as L
    from deep_rl_battlespace_amd import learner
    hdr = open(os.path.join(ROOT, "include", "battlespace_hip.h")).read()
    lib = L.load()
    for name in ("bsx_shuffle_rows", "bsx_minibatch_gather"):
        assert re.search(r"^int " + name + r"\(", hdr, flags=re.M) and name in L.SIGNATURES and hasattr(lib, name)
    assert lib.bsx_abi_version() == 14 == L.ABI_VERSION
    fields = re.search(r"typedef struct BsxMinibatchIo \{(.*?)\} BsxMinibatchIo;", hdr, flags=re.S).group(1)
    assert re.findall(r"(\w+);", fields) == [f for f, _ in L.BsxMinibatchIo._fields_]
    assert ctypes.sizeof(L.BsxMinibatchIo) == 15 * 8
    build = open(os.path.join(ROOT, "deep-rl-battlespace_amd", "build.py")).read()
    assert re.search(r'"bsx_shuffle\.hip"\), \[\]\)', build)                       # no extra flags
    src = open(os.path.join(ROOT, "deep-rl-battlespace_amd", "csrc", "bsx_shuffle.hip")).read()
    assert int(re.search(r"constexpr int ROWS = (\d+);", src).group(1)) == learner.GATHER_ROWS
    assert "asm" not in src


def test_the_c_entry_points_refuse_what_the_header_documents_before_any_launch():
    """Fake addresses only: every call is refused before anything reaches HIP, argument rules before alignment rules."""
    from deep_rl_battlespace_amd import _lib as L
    lib = L.load()
    OK, A4, A1 = 4096, 4096 + 4, 4096 + 1
    ARG, ALIGN = -1, -2
    floats = [p + f for p in ("", "dst_") for f in L.MINIBATCH_FIELDS if f != "mask"]
    every = floats + ["mask", "dst_mask", "idx"]

    def gather(io=True, N=768, first=0, R=192, A=2, D=5, base=None, **kw):
        st = L.BsxMinibatchIo()
        for f in every:
            setattr(st, f, kw.get(f, OK))
        return lib.bsx_minibatch_gather(ctypes.byref(st) if io else None, N, first, R, A, D, 41, 7, base, None)

    arg = [dict(io=False)] + [{f: None} for f in every if f not in ("value", "dst_value")]
    arg += [dict(value=None), dict(dst_value=None)]                                # one side of value only
    arg += [dict(N=0), dict(N=-1), dict(N=2 ** 31), dict(R=0), dict(R=-5), dict(first=-1), dict(first=577), dict(first=768, R=1),
            dict(N=2 ** 31 - 1, first=2 ** 31 - 2, R=2), dict(first=2 ** 62, R=2 ** 62)]
    arg += [dict(A=0), dict(A=1), dict(A=3), dict(A=34), dict(A=-2), dict(D=0), dict(D=51), dict(D=-1)]
    for kw in arg:
        assert gather(**kw) == ARG, kw
    align = [{f: A1} for f in floats] + [{f: OK + 2} for f in floats] + [dict(idx=A4), dict(base=A4)]
    for kw in align:
        assert gather(**kw) == ALIGN, kw
    # the mask is bytes: any address; value on neither side is judged by the other fields alone
    assert gather(mask=A1, dst_mask=A1, obs=A1) == ALIGN
    assert gather(value=None, dst_value=None, idx=A4) == ALIGN
    # the order: argument rules before alignment rules, and within them null pointers, the row range, A, D
    for kw in (dict(obs=A1, R=0), dict(idx=A4, A=3), dict(base=A4, D=0), dict(dst_ret=A1, mask=None), dict(rec=A1, value=None)):
        assert gather(**kw) == ARG, kw

    def rows(N=768, first=0, R=192, base=None, idx=OK):
        return lib.bsx_shuffle_rows(N, first, R, 41, 7, base, idx, None)
    for kw in (dict(idx=None), dict(N=0), dict(N=2 ** 31), dict(R=0), dict(first=-1), dict(first=577), dict(first=768, R=1),
               dict(first=2 ** 62, R=2 ** 62), dict(idx=A4, R=0), dict(base=A4, N=0)):
        assert rows(**kw) == ARG, kw
    for kw in (dict(idx=A4), dict(idx=A1), dict(base=A4), dict(base=A1)):
        assert rows(**kw) == ALIGN, kw


def test_the_wrappers_name_the_argument_they_refuse():
    import torch
    from deep_rl_battlespace_amd import learner
    with pytest.raises(ValueError, match="N must be"):
        learner.shuffle_rows(0, 0, 1, 41, 7)
    with pytest.raises(ValueError, match="N must be"):
        learner.shuffle_rows(2 ** 31, 0, 1, 41, 7)
    for first, R in ((0, 0), (-1, 4), (765, 4)):
        with pytest.raises(ValueError, match="non-empty range"):
            learner.shuffle_rows(768, first, R, 41, 7)
    for seed, seq, name in ((-1, 7, "seed"), (2 ** 64, 7, "seed"), (41, -1, "seq"), (41.0, 7, "seed"), (True, 7, "seed")):
        with pytest.raises(ValueError, match=name):
            learner.shuffle_rows(768, 0, 4, seed, seq)
    with pytest.raises(ValueError, match="GPU"):
        learner.shuffle_rows(768, 0, 4, 41, 7, out=torch.zeros(4, dtype=torch.int64))
    f = lambda *s: torch.zeros(s)                                                   # noqa: E731
    src = learner.Minibatch(f(8, 2, 5), f(8, 2, 4), f(8, 2), f(8, 2), f(8, 2), torch.zeros(8, 2, dtype=torch.uint8))
    with pytest.raises(ValueError, match="GPU"):
        learner.minibatch_gather(src, src, 0, 4, 41, 7)
    with pytest.raises(ValueError, match=r"src\.obs"):
        learner.minibatch_gather(src._replace(obs=f(8, 3, 5)), src, 0, 4, 41, 7)
    assert learner.Minibatch._fields == ("obs", "rec", "logp", "adv", "ret", "mask", "value", "idx")


def test_the_learner_checks_its_shuffle_arguments_before_it_touches_a_device():
    """A stand-in rollout with what the constructor reads first: the shuffle arguments are refused by name; with good ones the
    constructor goes on to its device checks (the stand-in has no networks: an AttributeError, not a ValueError about shuffle)."""
    from deep_rl_battlespace_amd.learner import PPOLearner
    ro = types.SimpleNamespace(_sample=dict(temperature=0.7), _gauss=None, _value_w=object(), _gae=dict(), T=8, fused=types.SimpleNamespace(seed=41))
    for kw, name in ((dict(shuffle=1), "shuffle must be"), (dict(shuffle="yes"), "shuffle must be"), (dict(shuffle_seed=3), "shuffle_seed belongs"),
                     (dict(shuffle=True, shuffle_seed=-1), "shuffle_seed"), (dict(shuffle=True, shuffle_seed=2 ** 64), "shuffle_seed"),
                     (dict(shuffle=True, shuffle_seed=1.5), "shuffle_seed"), (dict(shuffle=True, minibatches=3), "divides T")):
        with pytest.raises(ValueError, match=name):
            PPOLearner(ro, **kw)
    for kw in (dict(shuffle=True), dict(shuffle=True, shuffle_seed=2 ** 64 - 1), dict()):
        with pytest.raises(AttributeError):
            PPOLearner(ro, **kw)
