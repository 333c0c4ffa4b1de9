"""CPU-side checks of the n-step fold (csrc/bsx_replay_nstep.hip, replay.NStepAppender): the properties of the numpy restatement that the
GPU tests hold the kernel to (tests/nstep_util.py), the C entry points' refusals before any launch (fake addresses only), and the Python
surface.  No kernel is launched here."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import nstep_util as U
from deep_rl_battlespace_amd import _lib
from deep_rl_battlespace_amd.replay import DeviceReplayBuffer, NStepAppender

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("bsx_replay_nstep_workspace_bytes", "bsx_replay_nstep_fold", "bsx_replay_nstep_carry")
ARG, ALIGN = -1, -2
A = 4096                      # a 256-byte aligned fake address (never dereferenced)
GAMMA = 0.95


def _fold_run(run, T, n, c0, nA, k, D, dtype=np.float32, gamma=GAMMA, reset=None):
    """The run's records through one NStepRef -> (list of folded row dicts, the ref).  reset: {call index: mask} for reset_carry before it."""
    ref = U.NStepRef(n, gamma, run["rew"].shape[1], nA, D, k, dtype)
    outs = []
    for c, rec in enumerate(U.chunks(run, T)):
        if reset and c in reset:
            ref.reset_carry(reset[c])
        outs.append(ref.fold(*U.team(rec, c0, nA, k)))
    return outs, ref


@pytest.mark.parametrize("T", [1, 4, 7])
def test_one_step_is_the_identity(T):
    E, nA, D, k, c0 = 16, 2, 5, 3, 1
    run = U.make_run(E, T, 1, nA + 2, D, down=c0)
    outs, ref = _fold_run(run, T, 1, c0, nA, k, D)
    for rec, out in zip(U.chunks(run, T), outs):
        obs, act, rew, done, ed = U.team(rec, c0, nA, k)
        for got, want in ((out["obs"], obs[:T]), (out["obs_next"], obs[1:]), (out["act"], act), (out["rew"], rew), (out["done"], done),
                          (out["skip"], ed[:T])):
            assert np.array_equal(U.bits(got), U.bits(want.reshape(got.shape)))
    assert ref.valid.all()


@pytest.mark.parametrize("n", [2, 3, 5])
def test_float64_returns_obey_the_recursion_where_no_agent_is_down(n):
    """R_n(t) = r_t + gamma * R_{n-1}(t + 1) on games that never end.  Both sides are float64 sums of the same n terms in a different
    order, each of at most n roundings of relative size 2^-53: they agree within 2 n 2^-53 sum_j |gamma^j r_{t+j}| <= 2 n 2^-53 sum |r|."""
    E, T, nA, D, k = 4, 9, 2, 3, 3
    run = U.make_run(E, T, n, nA, D, calls=1, shift=7)                 # SCENARIOS[7] first: games 0 is "never ends"
    run = {key: np.repeat(v[:, :1], E, axis=1) for key, v in run.items()}
    assert not run["done"].any() and not run["env_done"].any()
    rec = U.chunks(run, T)[0]
    full = U.NStepRef(n, GAMMA, E, nA, D, k, np.float64).fold(*U.team(rec, 0, nA, k))
    less = U.NStepRef(n - 1, GAMMA, E, nA, D, k, np.float64).fold(*U.team(rec, 0, nA, k))
    # fresh carries: the call emits timeline ticks u = 0 .. T-1, of which u >= n - 1 are the record's ticks t = u - (n - 1)
    Rn = full["rew"].reshape(T, E, nA)[n - 1:]                          # t = 0 .. T - n
    Rn1 = less["rew"].reshape(T, E, nA)[n - 2:][1:T - n + 2]            # t + 1 = 1 .. T - n + 1
    r = rec["rew"].astype(np.float64)
    want = r[:T - n + 1] + GAMMA * Rn1
    bound = 2 * n * 2.0 ** -53 * sum(np.abs(r[j:T - n + 1 + j]) for j in range(n))
    print("largest difference", np.abs(Rn - want).max(), "bound", bound.min())
    assert (np.abs(Rn - want) <= bound).all()
    assert (full["m"].reshape(T, E)[n - 1:] == n).all() and not full["done"].reshape(T, E, nA)[n - 1:].any()


@pytest.mark.parametrize("n,T", [(2, 2), (3, 3), (3, 4), (5, 7), (1, 3)])
def test_chunking_a_run_does_not_change_the_rows_or_their_order(n, T):
    E, nA, D, k, c0 = 16, 2, 4, 4, 1
    run = U.make_run(E, T, n, nA + 1, D, calls=2, down=c0)
    halves, ref2 = _fold_run(run, T, n, c0, nA, k, D)
    whole, ref1 = _fold_run(run, 2 * T, n, c0, nA, k, D)
    for f in U.RING_FIELDS + ("skip", "m"):
        assert np.array_equal(U.bits(np.concatenate([h[f] for h in halves])), U.bits(whole[0][f])), f
    for f in ("c_obs", "c_act", "c_rew", "c_done", "c_ed", "valid"):
        assert np.array_equal(U.bits(getattr(ref1, f)), U.bits(getattr(ref2, f))), f


@pytest.mark.parametrize("n,T", [(2, 2), (3, 4), (5, 7)])
def test_a_window_cut_short_sets_every_agents_done(n, T):
    E, nA, D, k = 16, 3, 3, 3
    run = U.make_run(E, T, n, nA, D)
    outs, _ = _fold_run(run, T, n, 0, nA, k, D)
    short = np.concatenate([o["m"] < n for o in outs])
    done = np.concatenate([o["done"] for o in outs])
    skip = np.concatenate([o["skip"] for o in outs])
    assert short.any() and (~short).any() and (skip == 0).any()
    assert done[short].all()
    # and the hand-made record holds what it promises: an agent down before its game's end, with rewards recorded after it
    assert (done.any(1) & ~done.all(1) & (skip == 0)).any()


def test_reset_carry_drops_exactly_the_masked_games_carried_ticks():
    E, T, n, nA, D, k = 16, 5, 3, 2, 3, 3
    run = U.make_run(E, T, n, nA, D, shift=7)
    mask = np.zeros(E, bool)
    mask[[1, 4, 9]] = True
    plain, _ = _fold_run(run, T, n, 0, nA, k, D)
    reset, _ = _fold_run(run, T, n, 0, nA, k, D, reset={1: mask})
    carried = np.zeros((T, E), bool)
    carried[:n - 1] = True
    want = plain[1]["skip"].reshape(T, E).astype(bool) | (carried & mask)
    assert np.array_equal(reset[1]["skip"].reshape(T, E).astype(bool), want)
    assert (want != plain[1]["skip"].reshape(T, E).astype(bool)).any()
    for f in U.RING_FIELDS:                                  # nothing else changes, and the call after it is the plain one
        assert np.array_equal(U.bits(reset[1][f]), U.bits(plain[1][f])) and np.array_equal(U.bits(reset[2][f]), U.bits(plain[2][f]))
    assert np.array_equal(reset[2]["skip"], plain[2]["skip"])


def test_nstep_symbols_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "battlespace_hip.h")).read()
    declared = set(re.findall(r"^\s*int\s+(bsx_\w+)\s*\(", hdr, flags=re.M))
    lib = _lib.load()
    for name in NAMES:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.bsx_abi_version() == 14                 # additive: the ABI version stays


def test_workspace_bytes_and_its_refusals():
    lib = _lib.load()
    sz = ctypes.c_size_t()
    for (T, E, nA, D, k, n) in ((3, 1, 1, 5, 3, 3), (7, 257, 3, 11, 4, 5), (32, 65536, 1, 5, 4, 3)):
        assert lib.bsx_replay_nstep_workspace_bytes(T, E, nA, D, k, n, ctypes.byref(sz)) == 0
        assert sz.value == T * E * nA * (4 * (2 * D + k + 1) + 1) + T * E
    ok = dict(T=8, E=64, nA=2, D=8, k=4, n=3)
    for bad in (dict(n=0), dict(n=17), dict(n=9), dict(T=0), dict(T=65536), dict(E=0), dict(E=1 << 31), dict(T=65535, E=1 << 16), dict(nA=0),
                dict(nA=17), dict(D=0), dict(D=51), dict(k=2), dict(k=5)):
        a = dict(ok, **bad)
        assert lib.bsx_replay_nstep_workspace_bytes(a["T"], a["E"], a["nA"], a["D"], a["k"], a["n"], ctypes.byref(sz)) == ARG, bad
    assert lib.bsx_replay_nstep_workspace_bytes(8, 64, 2, 8, 4, 3, None) == ARG


def _source(**kw):
    f = dict(obs=A, obs_row=32, obs_col=8, obs_next=None, obs_next_row=0, obs_next_col=0, act=A, act_row=16, act_col=4,
             rew=A, rew_row=4, rew_col=1, done=A, done_row=4, done_col=1, skip=A, skip_row=1)
    f.update(kw)
    return _lib.BsxReplaySource(*(f[name] for name, _ in _lib.BsxReplaySource._fields_))


def _carry(**kw):
    f = dict(obs=A, act=A, rew=A, done=A, env_done=A, valid=A)
    f.update(kw)
    return _lib.BsxNstepCarry(*(f[name] for name, _ in _lib.BsxNstepCarry._fields_))


def _cases():
    cases = [(ARG, dict(no_src=True)), (ARG, dict(no_carry=True))]
    cases += [(ARG, dict(shape=kw)) for kw in (dict(n=0), dict(n=17), dict(T=2), dict(E=0), dict(nA=17), dict(D=51), dict(k=5))]
    cases += [(ARG, dict(src={f: None})) for f in ("obs", "act", "rew", "done", "skip")]
    cases += [(ARG, dict(src={f: -1})) for f in ("obs_row", "obs_col", "act_row", "act_col", "rew_row", "rew_col", "done_row", "done_col", "skip_row")]
    cases += [(ARG, dict(carry={f: None})) for f in ("obs", "act", "rew", "done", "env_done", "valid")]
    cases += [(ALIGN, dict(src={f: A + 2})) for f in ("obs", "act", "rew")] + [(ALIGN, dict(carry={f: A + 2})) for f in ("obs", "act", "rew")]
    # two rules broken at once: every BSX_E_ARG is found before any BSX_E_ALIGN
    cases += [(ARG, dict(src=dict(obs=A + 2), shape=dict(n=0))), (ARG, dict(carry=dict(rew=A + 2, valid=None))),
              (ARG, dict(src=dict(act=A + 2, done_col=-1)))]
    return cases


def test_fold_and_carry_reject_bad_arguments_before_any_launch():
    """Every case ends in a refusal: a call that got through would launch on a machine that may have no GPU.  The record's obs_next is
    NULL throughout: it is not read."""
    lib = _lib.load()

    def call(entry, src=None, carry=None, shape=None, no_src=False, no_carry=False, gamma=0.9, ws=A, folded=True):
        s = None if no_src else ctypes.byref(_source(**(src or {})))
        c = None if no_carry else ctypes.byref(_carry(**(carry or {})))
        a = dict(dict(T=8, E=64, nA=2, D=8, k=4, n=3), **(shape or {}))
        dims = (a["T"], a["E"], a["nA"], a["D"], a["k"], a["n"])
        if entry == "carry":
            return lib.bsx_replay_nstep_carry(s, c, *dims, None)
        out = _lib.BsxReplaySource()
        return lib.bsx_replay_nstep_fold(s, c, *dims, gamma, ws, ctypes.byref(out) if folded else None, None)

    for want, kw in _cases():
        assert call("fold", **kw) == want, kw
        assert call("carry", **kw) == want, kw
    for kw in (dict(gamma=-0.1), dict(gamma=1.5), dict(gamma=float("nan")), dict(ws=None), dict(folded=False),
               dict(gamma=2.0, ws=A + 2), dict(ws=None, src=dict(rew=A + 2))):
        assert call("fold", **kw) == ARG, kw
    assert call("fold", ws=A + 2) == ALIGN
    # n = 1: the carry is empty, only `valid` is needed
    empty = dict(obs=None, act=None, rew=None, done=None, env_done=None)
    assert call("fold", carry=empty, shape=dict(n=1), ws=A + 2) == ALIGN              # (got past every BSX_E_ARG)
    assert call("fold", carry=dict(empty, valid=None), shape=dict(n=1)) == ARG
    assert call("carry", carry=dict(empty, valid=None), shape=dict(n=1)) == ARG


def _buf(nA=2, D=8, k=4, M=64):
    return DeviceReplayBuffer(M, 4, [f"plane{i}" for i in range(nA)], D, D * nA, k, device="cpu")


def test_appender_surface():
    buf = _buf()
    app = NStepAppender(buf, n=3, gamma=0.95, T=8, E=5)
    assert app.n_step == 3 and app.gamma == 0.95 and app.buf is buf
    assert app.bootstrap_gamma == float(U.gamma_chain(0.95, 3)[3]) and NStepAppender(buf, 1, 0.5, 8, 5).bootstrap_gamma == 0.5
    assert app.carry_valid.dtype == torch.uint8 and tuple(app.carry_valid.shape) == (5,) and not app.carry_valid.any()
    app.carry_valid.fill_(1)
    app.reset_carry(torch.tensor([True, False, False, True, False]))
    assert app.carry_valid.tolist() == [0, 1, 1, 0, 1]
    app.reset_carry()
    assert not app.carry_valid.any()
    with pytest.raises(ValueError):
        app.reset_carry(torch.ones(4, dtype=torch.bool))
    for kw in (dict(n=0), dict(n=17), dict(n=9), dict(gamma=-0.1), dict(gamma=1.01), dict(gamma=float("nan")), dict(E=0)):
        with pytest.raises(ValueError):
            NStepAppender(buf, **dict(dict(n=3, gamma=0.95, T=8, E=5), **kw))
    with pytest.raises(ValueError):
        NStepAppender(object(), 3, 0.95, 8, 5)
    # nothing is allocated after construction: the ring's own append workspace for T * E rows is there already
    need = _lib.query_bytes("bsx_replay_workspace_bytes", 8 * 5)
    assert buf._workspaces[-1].numel() * 8 >= need


def test_append_refuses_a_record_that_does_not_fit_the_constructor():
    buf = _buf(nA=2, D=8, k=4)
    T, E, Aw = 8, 5, 4
    app = NStepAppender(buf, n=3, gamma=0.95, T=T, E=E)

    def rec(T=T, E=E, D=8, Aw=Aw):
        return dict(obs=torch.zeros(T + 1, E, Aw, D), act=torch.zeros(T, E, Aw, 4), rew=torch.zeros(T, E, Aw),
                    done=torch.zeros(T, E, Aw, dtype=torch.uint8), env_done=torch.zeros(T + 1, E, dtype=torch.uint8))

    bad = [rec(T=7), rec(E=6), rec(D=9), dict(rec(), rew=torch.zeros(T, E, Aw, dtype=torch.float64)), dict(rec(), done=torch.zeros(T, E, Aw)),
           dict(rec(), env_done=torch.zeros(T, E, dtype=torch.uint8)), dict(rec(), act=torch.zeros(T, E, Aw, 4)[..., :3])]
    for r in bad:
        with pytest.raises(ValueError):
            app.append(r["obs"], r["act"], r["rew"], r["done"], r["env_done"], range(2))
    for cols in (range(3), [0, 2], range(3, 5), []):
        r = rec()
        with pytest.raises(ValueError):
            app.append(r["obs"], r["act"], r["rew"], r["done"], r["env_done"], cols)

    class Rollout:
        T = 7
    with pytest.raises(ValueError):
        app.append_rollout(Rollout(), range(2))
