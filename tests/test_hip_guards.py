"""Every device entry point at ragged sizes -- tiny batches and batches that are not a multiple of a workgroup's games -- with each of
its buffers inside a guard slab (guard_util.Buffers): no call writes a byte outside its buffers, the state block's alignment padding
and the pools that hold no game stay zero, and every output is bit-identical to the same calls on exactly-sized buffers.  The fused
rollout is also compared with its per-tick two-kernel form, and at 5 x 4v4 and 7 x 3v3 with the C oracle.  Driven through ctypes.
Where such a call READS beyond its buffers no result changes; that is checked without a GPU (test_footprint_cpu.py)."""
import ctypes

import numpy as np
import pytest
import torch

from gae_util import gae_ref
from guard_util import STATE_PAD, Buffers, group_width, layout, pools
from oracle import cref
from trace_util import OBS_ATOL, OBS_RTOL

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 3, 5, 7, 9, 17, 31, 33, 63, 65, 255, 257, 489)
SEED = 11
f32, f64, u8, i32, i64 = torch.float32, torch.float64, torch.uint8, torch.int32, torch.int64


def _L():
    from deep_rl_battlespace_amd import _lib
    return _lib


def _ok(rc, what):
    _L().check(rc, what)


def _s():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.detach().reshape(-1).contiguous().view(torch.uint8)


def _assert_same(got, want, what, skip=()):
    a, b = [r for r in got if r[0] not in skip], [r for r in want if r[0] not in skip]
    assert [r[0] for r in a] == [r[0] for r in b], what
    for (name, x), (_, y) in zip(a, b):
        assert x.shape == y.shape and torch.equal(_bits(x), _bits(y)), (what, name)


def _state(buf, E, n):
    lib = _L().load()
    nb = ctypes.c_size_t()
    _ok(lib.bsx_state_bytes(E, n, ctypes.byref(nb)), "bsx_state_bytes")
    st = buf("state", nb.value, u8, 0, pad=STATE_PAD)
    _ok(lib.bsx_state_init(st.data_ptr(), E, n, _s()), "bsx_state_init")
    return st


def _assert_padding_zero(st, E, n):
    """The bytes between the fields of make_layout are zero, and so are the pools beyond the games' own blocks (count and entries)."""
    fields, total = layout(E, n)
    assert st.numel() == total, (E, n)
    h = st.cpu().numpy()
    for i, (name, off, used) in enumerate(fields):
        end = fields[i + 1][1] if i + 1 < len(fields) else total
        assert not h[off + used:end].any(), ("padding after", name, E, n)
    own, nb = -(-E // (64 // group_width(n))), pools(E, n)
    off = dict((f, o) for f, o, _ in fields)
    assert not h[off["bcnt"] + 4 * own:off["bcnt"] + 4 * nb].any(), ("counts of the pools beyond the games", E, n)
    assert not h[off["bent"] + 6144 * own:off["bent"] + 6144 * nb].any(), ("entries of the pools beyond the games", E, n)


def _export(buf, lib, st, E, n, keep, tag="x"):
    EA = E * 2 * n
    shapes = dict(px=(EA, i32), py=(EA, i32), pdir=(EA, f64), php=(EA, i32), palive=(EA, u8), base_xy=(4 * E, i32), bhp=(2 * E, i32),
                  tick=(E, i32), env_done=(E, u8), winner=(E, u8), bl_live=(12 * EA, u8), bl_x=(12 * EA, i32), bl_y=(12 * EA, i32),
                  bl_dir=(12 * EA, f64), counters=(4 * E, i32))
    L = _L()
    out = {f: buf(f"{tag}_{f}", shapes[f][0], shapes[f][1], 0) for f in L.EXPORT_FIELDS}
    ex = L.BsxExport(*[out[f].data_ptr() for f in L.EXPORT_FIELDS])
    _ok(lib.bsx_export_state(st.data_ptr(), E, n, ctypes.byref(ex), _s()), "bsx_export_state")
    for f in L.EXPORT_FIELDS:
        keep(f"{tag}_{f}", out[f])


def _actions(g, EA, kind, cont, T=None):
    """Host actions of one call (or T calls): mostly shots (discrete), [-1.2, 1.2] rows (continuous: clipped in the kernel)."""
    L, lead = _L(), (() if T is None else (T,))
    if not cont and kind == L.ACT_I32:
        a = torch.randint(0, 5, lead + (EA,), generator=g, dtype=i32)
        return torch.where(torch.rand(lead + (EA,), generator=g) < 0.6, torch.ones_like(a), a)
    if not cont:
        return torch.randn(lead + (EA * 4,), generator=g)
    w = 4 if kind == L.ACT_F32X4 else 3
    return (torch.rand(lead + (EA * w,), generator=g, dtype=f64) * 2.4 - 1.2).to(f64 if kind == L.ACT_F64 else f32)


def _play_steps(buf, E, n, cont):
    """init, reset, three per-call steps (every action encoding of the family, one with injected jitters), a masked reset, observe,
    two multi-tick launches (store_all 1 and 0), range launches, export, the scripted-opponent kernels.  -> (records, state)."""
    L = _L()
    lib, s = L.load(), _s()
    A, D = 2 * n, 3 * n + 2
    EA = E * A
    cfg, flags = L.BsxRewards(100, 10, -1, -5, -20), L.F_AUTO_RESET
    g = torch.Generator().manual_seed(100 * E + n)
    rec = []

    def keep(name, t):
        rec.append((name, t.clone()))
    st = _state(buf, E, n)
    P = st.data_ptr()
    obs, rew, done = buf("obs", EA * D, f32, -7.0), buf("rew", EA, f32, -7.0), buf("done", EA, u8, 7)
    env_done, winner = buf("env_done", E, u8, 7), buf("winner", E, u8, 7)

    def keep_out(tag):
        for name, t in (("obs", obs), ("rew", rew), ("done", done), ("env_done", env_done), ("winner", winner)):
            keep(f"{tag} {name}", t)
    _ok(lib.bsx_reset(P, E, n, None, None, SEED, 1, 0, obs.data_ptr(), s), "bsx_reset")
    keep("reset obs", obs)
    step = lib.bsx_step_continuous if cont else lib.bsx_step_discrete
    kinds = (L.ACT_F32, L.ACT_F64, L.ACT_F32X4) if cont else (L.ACT_I32, L.ACT_LOGITS_F32, L.ACT_I32)
    acts = []
    for k, kind in enumerate(kinds):
        host = _actions(g, EA, kind, cont)
        act = buf(f"act{k}", host.numel(), host.dtype)
        act.copy_(host)
        acts.append(act)
        u = None
        if k == 1:
            u = buf("u", EA, f64)
            u.copy_(torch.rand(EA, generator=g, dtype=f64))
        _ok(step(P, E, n, act.data_ptr(), kind, None if u is None else u.data_ptr(), obs.data_ptr(), rew.data_ptr(), done.data_ptr(),
                 env_done.data_ptr(), winner.data_ptr(), ctypes.byref(cfg), flags, SEED, 0, s), "bsx_step")
        keep_out(f"step{k}")
    mask = buf("mask", E, u8)
    mask.copy_((torch.arange(E) % 3 == 1).to(u8))
    _ok(lib.bsx_reset(P, E, n, mask.data_ptr(), None, SEED, 2, 0, obs.data_ptr(), s), "bsx_reset masked")
    keep("masked reset obs", obs)
    obs2 = buf("obs2", EA * D, f32, -7.0)
    _ok(lib.bsx_observe(P, E, n, obs2.data_ptr(), s), "bsx_observe")
    keep("observe", obs2)
    many = lib.bsx_step_many_continuous if cont else lib.bsx_step_many_discrete
    mkind = L.ACT_F64 if cont else L.ACT_I32
    T = 5
    host = _actions(g, EA, mkind, cont, T)
    am = buf("act_many", host.numel(), host.dtype)
    am.copy_(host.reshape(-1))
    obs_t, rew_t, done_t = buf("obs_t", T * EA * D, f32, -7.0), buf("rew_t", T * EA, f32, -7.0), buf("done_t", T * EA, u8, 7)
    edt = buf("env_done_t", T * E, u8, 7)
    _ok(many(P, E, n, T, am.data_ptr(), mkind, None, obs_t.data_ptr(), rew_t.data_ptr(), done_t.data_ptr(), env_done.data_ptr(),
             winner.data_ptr(), edt.data_ptr(), ctypes.byref(cfg), flags, 1, SEED, 0, s), "bsx_step_many store_all")
    for name, t in (("obs_t", obs_t), ("rew_t", rew_t), ("done_t", done_t), ("env_done_t", edt), ("env_done", env_done), ("winner", winner)):
        keep(f"many1 {name}", t)
    um = buf("u_many", 3 * EA, f64)
    um.copy_(torch.rand(3 * EA, generator=g, dtype=f64))
    _ok(many(P, E, n, 3, am.data_ptr(), mkind, um.data_ptr(), obs.data_ptr(), rew.data_ptr(), done.data_ptr(), None, None, None,
             ctypes.byref(cfg), flags, 0, SEED, 0, s), "bsx_step_many last tick only")
    keep_out("many0")
    # one launch past the time-limit tie: every game ends at least once (auto-reset, the counters' atomics, a finished game's pool)
    TL = lib.bsx_tie_tick(n) + 3
    lkind = L.ACT_F32 if cont else L.ACT_I32
    host = _actions(g, EA, lkind, cont, TL)
    al, edl = buf("act_long", host.numel(), host.dtype), buf("env_done_long", TL * E, u8, 7)
    al.copy_(host.reshape(-1))
    _ok(many(P, E, n, TL, al.data_ptr(), lkind, None, obs.data_ptr(), rew.data_ptr(), done.data_ptr(), env_done.data_ptr(), winner.data_ptr(),
             edl.data_ptr(), ctypes.byref(cfg), flags, 0, SEED, 0, s), "bsx_step_many past the tie")
    keep_out("long")
    keep("long env_done_t", edl)
    rng = lib.bsx_step_continuous_range if cont else lib.bsx_step_discrete_range
    for first, count in [(0, (E + 1) // 2)] + ([(256, E - 256)] if E > 256 else []):
        _ok(rng(P, E, n, first, count, acts[0].data_ptr(), kinds[0], None, obs.data_ptr(), rew.data_ptr(), done.data_ptr(),
                env_done.data_ptr(), winner.data_ptr(), ctypes.byref(cfg), flags, SEED, 0, s), "bsx_step_range")
        keep_out(f"range {first}+{count}")
    _export(buf, lib, st, E, n, keep)
    # the scripted opponent on the last observations: int32 and one-hot rows, continuous rows with Philox or given draws, the _shard entry
    ia, il = buf("inst_i32", EA, i32, -9), buf("inst_onehot", EA * 4, f32, -9.0)
    _ok(lib.bsx_instinct_discrete(obs.data_ptr(), ia.data_ptr(), L.ACT_I32, E, n, 1, s), "bsx_instinct_discrete")
    _ok(lib.bsx_instinct_discrete(obs.data_ptr(), il.data_ptr(), L.ACT_LOGITS_F32, E, n, 2, s), "bsx_instinct_discrete one-hot")
    ic, ics = buf("inst_cont", EA * 3, f64, -9.0), buf("inst_shard", EA * 3, f64, -9.0)
    rnd, sb = buf("inst_rnd", EA * 4, f64), buf("inst_seq_base", 1, i64, 4)
    rnd.copy_(torch.rand(EA * 4, generator=g, dtype=f64))
    _ok(lib.bsx_instinct_continuous(obs.data_ptr(), ic.data_ptr(), None, E, n, 0, 5, 3, None, s), "bsx_instinct_continuous")
    _ok(lib.bsx_instinct_continuous_shard(obs.data_ptr(), ics.data_ptr(), rnd.data_ptr() if E % 2 else None, E, n, 2, 5, 3, sb.data_ptr(),
                                          1000, s), "bsx_instinct_continuous_shard")
    for name, t in (("inst_i32", ia), ("inst_onehot", il), ("inst_cont", ic), ("inst_shard", ics)):
        keep(name, t)
    keep("state", st)
    return rec, st


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 8, 16])
def test_step_observe_reset_export_and_scripted_calls_stay_inside_their_buffers(n):
    """Per-call, multi-tick (store_all 0 / 1), range (first 0 and 256, ragged counts), masked-reset, observe, export and scripted-opponent
    calls at every ragged size; discrete and continuous alternate over the sizes (and flip with n)."""
    lib = _L().load()
    for i, E in enumerate(SIZES):
        cont = (i + n) % 2 == 1
        guarded = Buffers(True)
        got, st = _play_steps(guarded, E, n, cont)
        want, st_w = _play_steps(Buffers(False), E, n, cont)
        torch.cuda.synchronize()
        assert not guarded.stray(), ("writes outside the buffers", E, n, cont, guarded.stray())
        _assert_same(got, want, (E, n, cont))
        _assert_padding_zero(st, E, n)
        assert bool((dict(got)["x_counters"].view(E, 4)[:, 0] >= 1).all()), ("every game has ended", E, n)
        for t in (st, st_w):
            _ok(lib.bsx_state_release(t.data_ptr()), "bsx_state_release")


def _actor_blobs(n, cont, heads):
    from deep_rl_battlespace_amd.rollout import StackedActor
    A, D = 2 * n, 3 * n + 2
    torch.manual_seed(7 * n + cont)
    actor = StackedActor(A, D, 3 if cont else 4, device="cuda")
    with torch.no_grad():
        actor.w3.mul_(60.0)
    w = actor.pack().reshape(-1)
    if not heads:
        return w, None
    critic = StackedActor(A, D, 1, device="cuda")
    with torch.no_grad():
        critic.w3.mul_(100.0)
    return w, critic.pack().reshape(-1)


def _rollout(buf, E, n, cont, var, blobs, one_launch, T=100, runs=2):
    """Two rollouts of T ticks from a reset (200 ticks: past the time-limit tie of every team size): one bsx_rollout_* launch each, or T x (bsx_actor_forward -> [scripted opponent] -> bsx_step_*)
    as rollout.PolicyRollout's per-tick form enqueues them.  -> (records, state, score rows of every run)."""
    L = _L()
    lib, s = L.load(), _s()
    A, D = 2 * n, 3 * n + 2
    EA = E * A
    cfg, flags = L.BsxRewards(100, 10, -1, -5, -20), L.F_AUTO_RESET
    rec, scored = [], []

    def keep(name, t):
        rec.append((name, t.clone()))
    st = _state(buf, E, n)
    P = st.data_ptr()
    w = buf("weights", blobs[0].numel(), f32)
    w.copy_(blobs[0])
    obs = buf("obs", (T + 1, EA * D), f32, -7.0)
    scores, rew, done = buf("scores", (T, EA * 4), f32, -7.0), buf("rew", (T, EA), f32, -7.0), buf("done", (T, EA), u8, 7)
    env_done, winner, edt = buf("env_done", E, u8, 7), buf("winner", E, u8, 7), buf("env_done_t", (T, E), u8, 7)
    seq_base = buf("seq_base", 1, i64, 0)
    nz = L.BsxActorNoise()
    heads = blobs[1] is not None
    if var["noise"] == "gauss":
        nz.gaussian_std = 0.3
    elif var["noise"] == "ou":
        ou = buf("ou_state", EA * 4, f32, 0.0)
        nz.ou_scale, nz.ou_theta, nz.ou_sigma, nz.ou_mu, nz.ou_state, nz.ou_keep = 0.3, 0.15, 0.2, 0.0, ou.data_ptr(), 0
    if heads:
        logp, value = buf("logp", (T, EA), f32, -7.0), buf("value", (T, EA), f32, -7.0)
        vw = buf("value_weights", blobs[1].numel(), f32)
        vw.copy_(blobs[1])
        nz.sample_mode, nz.temperature, nz.value_weights = 1, 0.7, vw.data_ptr()
    team = var["scripted"]
    act64 = buf("act64", (E, A, 3), f64, 0.0) if (cont and team >= 0 and not one_launch) else None
    prev = buf("env_done_before", E, u8, 0)                       # the per-tick form's OU restarts: env_done before the tick
    _ok(lib.bsx_reset(P, E, n, None, None, SEED, 1, 0, obs[0].data_ptr(), s), "bsx_reset")
    for r in range(runs):
        if r:
            obs[0].copy_(obs[T])
        if one_launch:
            if heads:
                nz.logp, nz.value = logp.data_ptr(), value.data_ptr()
            head = (P, E, n, T, w.data_ptr(), L.ACTOR_F32, team) + ((SEED + 1,) if cont else ())
            _ok((lib.bsx_rollout_continuous if cont else lib.bsx_rollout_discrete)(
                *head, obs.data_ptr(), scores.data_ptr(), rew.data_ptr(), done.data_ptr(), env_done.data_ptr(), winner.data_ptr(),
                edt.data_ptr(), ctypes.byref(cfg), flags, ctypes.byref(nz), 3, 0, seq_base.data_ptr(), SEED, 0, s), "bsx_rollout")
        else:
            for t in range(T):
                if var["noise"] == "ou":
                    nz.env_done = prev.data_ptr()
                if heads:
                    nz.logp, nz.value = logp[t].data_ptr(), value[t].data_ptr()
                _ok(lib.bsx_actor_forward(w.data_ptr(), obs[t].data_ptr(), scores[t].data_ptr(), E, n, L.ACTOR_F32, ctypes.byref(nz), 3, t,
                                          seq_base.data_ptr(), 0, s), "bsx_actor_forward")
                sc = scores[t].view(E, A, 4)
                act, kind = scores[t].data_ptr(), L.ACT_F32X4 if cont else L.ACT_LOGITS_F32
                if team >= 0 and not cont:
                    _ok(lib.bsx_instinct_discrete(obs[t].data_ptr(), act, L.ACT_LOGITS_F32, E, n, team, s), "bsx_instinct_discrete")
                elif team >= 0:
                    cols = slice(team * n, team * n + n)
                    act64.copy_(sc[..., :3])
                    _ok(lib.bsx_instinct_continuous_shard(obs[t].data_ptr(), act64.data_ptr(), None, E, n, team, SEED + 1, t,
                                                          seq_base.data_ptr(), 0, s), "bsx_instinct_continuous_shard")
                    sc[:, cols, :3] = act64[:, cols].float()
                    sc[:, cols, 3] = 0.0
                    act, kind = act64.data_ptr(), L.ACT_F64
                _ok((lib.bsx_step_continuous if cont else lib.bsx_step_discrete)(
                    P, E, n, act, kind, None, obs[t + 1].data_ptr(), rew[t].data_ptr(), done[t].data_ptr(), edt[t].data_ptr(),
                    winner.data_ptr(), ctypes.byref(cfg), flags, SEED, 0, s), "bsx_step")
                prev.copy_(edt[t])
            env_done.copy_(edt[T - 1])
        seq_base.add_(T)
        outs = [("obs", obs), ("scores", scores), ("rew", rew), ("done", done), ("env_done", env_done), ("winner", winner), ("env_done_t", edt)]
        if heads:
            outs += [("logp", logp), ("value", value)]
        if var["noise"] == "ou":
            outs.append(("ou_state", ou))
        for name, t in outs:
            keep(f"run{r} {name}", t)
        scored.append((scores.clone(), obs.clone(), rew.clone(), done.clone(), edt.clone()))
        _export(buf, lib, st, E, n, keep, tag=f"run{r} x")
    keep("state", st)
    return rec, st, scored


def _assert_c_oracle_plays_the_recorded_rows(E, n, scored):
    """The C oracle, stepping on the recorded score rows (arg-max), plays the same games: flags and rewards exact, observations to 1e-5."""
    c = cref.CRefBatch(E, n_agents=n, seed=SEED, auto_reset=True)
    o_c = c.reset()
    A = 2 * n
    for r, (sc, obs, rew, done, edt) in enumerate(scored):
        sc, obs, rew, done, edt = (x.cpu().numpy() for x in (sc, obs, rew, done, edt))
        T = sc.shape[0]
        if r == 0:
            np.testing.assert_allclose(obs[0].reshape(E, A, -1), o_c, rtol=OBS_RTOL, atol=OBS_ATOL)
        for t in range(T):
            co, cr, cd = c.step(sc[t].reshape(E, A, 4))
            assert np.array_equal(done[t].reshape(E, A).astype(bool), cd), (E, n, r, t)
            assert np.array_equal(rew[t].reshape(E, A).astype(np.float64), cr), (E, n, r, t)
            assert np.array_equal(edt[t], c.env_done), (E, n, r, t)
            np.testing.assert_allclose(obs[t + 1].reshape(E, A, -1), co, rtol=OBS_RTOL, atol=OBS_ATOL, err_msg=f"{E} x {n}v{n} run {r} tick {t}")


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_fused_rollouts_stay_inside_their_buffers_and_play_the_per_tick_games(n):
    """bsx_rollout_discrete / _continuous at every ragged size: Gaussian and OU noise, a scripted opponent on either side, and at 1v1 the
    categorical and value heads; two rollouts each.  Guards intact, padding and the game-less pools zero, bit-identical to the same
    calls on exactly-sized buffers and to the per-tick two-kernel form (whose state the C oracle pins elsewhere)."""
    lib = _L().load()
    for i, E in enumerate(SIZES):
        cases = [(cont, dict(noise=("ou" if (i + cont) % 3 == 1 else "gauss"), scripted=(-1 if (i + cont) % 3 != 2 else (i // 3) % 2)), False)
                 for cont in (False, True)]
        if n == 1:
            cases.append((False, dict(noise="none", scripted=-1), True))       # (a categorical head draws its own noise)
        for cont, var, heads in cases:
            blobs = _actor_blobs(n, cont, heads)
            guarded = Buffers(True)
            got, st, scored = _rollout(guarded, E, n, cont, var, blobs, True)
            want, st_w, _ = _rollout(Buffers(False), E, n, cont, var, blobs, True)
            tick, st_t, _ = _rollout(Buffers(False), E, n, cont, var, blobs, False)
            torch.cuda.synchronize()
            what = (E, n, cont, var, heads)
            assert not guarded.stray(), ("writes outside the buffers", what, guarded.stray())
            _assert_same(got, want, what)
            _assert_same(got, tick, ("per-tick form",) + what, skip=("state",))
            _assert_padding_zero(st, E, n)
            assert bool((dict(got)["run1 x_counters"].view(E, 4)[:, 0] >= 1).all()), ("every game has ended", what)
            if (E, n) in ((5, 4), (7, 3)) and not cont:
                _assert_c_oracle_plays_the_recorded_rows(E, n, scored)
            for t in (st, st_w, st_t):
                _ok(lib.bsx_state_release(t.data_ptr()), "bsx_state_release")


def _actor_forward(buf, E, n, precision, blobs):
    """bsx_actor_forward plain, then with Gaussian + OU noise (restarting the finished games' rows), the categorical head and the value head."""
    L = _L()
    lib, s = L.load(), _s()
    A, D = 2 * n, 3 * n + 2
    EA = E * A
    g = torch.Generator().manual_seed(E + 10 * n + 100 * precision)
    rec = []
    w, vw = buf("weights", blobs[0].numel(), f32), buf("value_weights", blobs[1].numel(), f32)
    w.copy_(blobs[0]); vw.copy_(blobs[1])
    obs = buf("obs", EA * D, f32)
    obs.copy_(torch.rand(EA * D, generator=g) * 2 - 0.5)
    sc1, sc2 = buf("scores_plain", EA * 4, f32, -7.0), buf("scores_noisy", EA * 4, f32, -7.0)
    ou, ed = buf("ou_state", EA * 4, f32), buf("env_done", E, u8)
    ou.copy_(torch.randn(EA * 4, generator=g)); ed.copy_((torch.arange(E) % 4 == 3).to(u8))
    logp, value, sb = buf("logp", EA, f32, -7.0), buf("value", EA, f32, -7.0), buf("seq_base", 1, i64, 9)
    _ok(lib.bsx_actor_forward(w.data_ptr(), obs.data_ptr(), sc1.data_ptr(), E, n, precision, None, 3, 1, None, 0, s), "bsx_actor_forward")
    nz = L.BsxActorNoise()
    nz.gaussian_std, nz.ou_scale, nz.ou_theta, nz.ou_sigma, nz.ou_state, nz.env_done = 0.2, 0.3, 0.15, 0.2, ou.data_ptr(), ed.data_ptr()
    nz.sample_mode, nz.temperature, nz.logp, nz.value_weights, nz.value = 1, 0.7, logp.data_ptr(), vw.data_ptr(), value.data_ptr()
    _ok(lib.bsx_actor_forward(w.data_ptr(), obs.data_ptr(), sc2.data_ptr(), E, n, precision, ctypes.byref(nz), 3, 2, sb.data_ptr(), 64, s),
        "bsx_actor_forward noisy")
    for name, t in (("scores_plain", sc1), ("scores_noisy", sc2), ("ou_state", ou), ("logp", logp), ("value", value)):
        rec.append((name, t.clone()))
    return rec


def test_actor_forward_stays_inside_its_buffers():
    """bsx_actor_forward at E = 1, 31, 33, 97 games of 1v1 ... 4v4 in all three precisions: a row block of the kernel is not a multiple
    of these."""
    L = _L()
    for n in (1, 2, 3, 4):
        blobs = _actor_blobs(n, False, True)
        for E in (1, 31, 33, 97):
            for precision in (L.ACTOR_F32, L.ACTOR_BF16X3, L.ACTOR_BF16X6):
                guarded = Buffers(True)
                got = _actor_forward(guarded, E, n, precision, blobs)
                want = _actor_forward(Buffers(False), E, n, precision, blobs)
                torch.cuda.synchronize()
                assert not guarded.stray(), ("writes outside the buffers", E, n, precision, guarded.stray())
                _assert_same(got, want, (E, n, precision))


def _gae(buf, T, E, A, normalize, case, agents=None):
    L = _L()
    lib = L.load()
    rew, value, done, env_done, lv, prev = (buf(k, v.numel(), v.dtype) for k, v in
                                            zip(("rew", "value", "done", "env_done", "last_value", "done_prev"), case))
    for b, v in zip((rew, value, done, env_done, lv, prev), case):
        b.copy_(v.reshape(-1))
    adv, ret, mask = buf("adv", T * E * A, f32, -7.0), buf("ret", T * E * A, f32, -7.0), buf("mask", T * E * A, u8, 7)
    ws = stats = None
    if normalize:
        nb = ctypes.c_size_t()
        _ok(lib.bsx_gae_workspace_bytes(E, A, T, ctypes.byref(nb)), "bsx_gae_workspace_bytes")
        ws, stats = buf("workspace", nb.value, u8, 0), buf("stats", 3, f64, -7.0)
    io = L.BsxGaeIo(rew.data_ptr(), value.data_ptr(), done.data_ptr(), env_done.data_ptr(), lv.data_ptr(), prev.data_ptr(), adv.data_ptr(),
                    ret.data_ptr(), mask.data_ptr())
    tail = (T, E, A, 0.97, 0.9, normalize, ws.data_ptr() if normalize else None, stats.data_ptr() if normalize else None, _s())
    if agents is None:
        _ok(lib.bsx_gae(ctypes.byref(io), *tail), "bsx_gae")
    else:                                                   # the flags behind ONE pad byte: a byte array takes any alignment
        on = buf("agent_on", A + 1, u8)[1:]
        on.copy_(agents)
        _ok(lib.bsx_gae_agents(ctypes.byref(io), on.data_ptr(), *tail), "bsx_gae_agents")
    return [(k, t.clone()) for k, t in (("adv", adv), ("ret", ret), ("mask", mask), ("done_prev", prev))] + \
        ([("stats", stats)] if normalize else [])


@pytest.mark.parametrize("T", [1, 9])
def test_gae_stays_inside_its_buffers_when_columns_are_not_a_multiple_of_four(T):
    """bsx_gae at E * A = 2 (mod 4) -- the kernel's 4-column vector path does not apply -- with and without the normalisation; without it
    the results are also the numpy restatement's, bit for bit."""
    g = torch.Generator().manual_seed(T)
    for E, A in ((1, 2), (3, 2), (33, 2), (489, 2), (7, 6), (17, 6)):
        assert E * A % 4 == 2
        case = (torch.randn((T, E, A), generator=g), torch.randn((T, E, A), generator=g), (torch.rand((T, E, A), generator=g) < 0.2).to(u8),
                (torch.rand((T + 1, E), generator=g) < 0.2).to(u8), torch.randn((E, A), generator=g), (torch.rand((E, A), generator=g) < 0.2).to(u8))
        for normalize in (0, 1):
            guarded = Buffers(True)
            got = _gae(guarded, T, E, A, normalize, case)
            want = _gae(Buffers(False), T, E, A, normalize, case)
            torch.cuda.synchronize()
            assert not guarded.stray(), ("writes outside the buffers", T, E, A, normalize, guarded.stray())
            _assert_same(got, want, (T, E, A, normalize))
            if not normalize:                                   # (the normalised path against it: test_hip_advantage.py)
                rew, value, done, env_done, lv, prev = (v.numpy() for v in case)
                adv, ret, mask, prev, _ = gae_ref(rew, value, lv, done, env_done, prev, 0.97, 0.9)
                r = {k: v.cpu().numpy() for k, v in got}
                assert np.array_equal(r["adv"].reshape(T, E, A), adv) and np.array_equal(r["ret"].reshape(T, E, A), ret), (T, E, A)
                assert np.array_equal(r["mask"].reshape(T, E, A).astype(bool), mask) and np.array_equal(r["done_prev"].reshape(E, A), prev), (T, E, A)
            # the same call with one team flagged off (bsx_gae_agents): nothing outside the buffers, the restatement's bits
            flag = torch.tensor([1] * (A // 2) + [0] * (A // 2), dtype=u8)
            guarded = Buffers(True)
            got = _gae(guarded, T, E, A, normalize, case, agents=flag)
            torch.cuda.synchronize()
            assert not guarded.stray(), ("writes outside the buffers", T, E, A, normalize, "agents", guarded.stray())
            rew, value, done, env_done, lv, prev = (v.numpy() for v in case)
            adv, ret, mask, prev, st = gae_ref(rew, value, lv, done, env_done, prev, 0.97, 0.9, bool(normalize), agents=flag.numpy(), kernel_order=True)
            r = {k: v.cpu().numpy() for k, v in got}
            assert np.array_equal(r["ret"].reshape(T, E, A).view(np.int32), ret.view(np.int32)), (T, E, A, "agents")
            assert np.array_equal(r["mask"].reshape(T, E, A).astype(bool), mask) and np.array_equal(r["done_prev"].reshape(E, A), prev), (T, E, A, "agents")
            assert np.array_equal(r["adv"].reshape(T, E, A).view(np.int32), adv.view(np.int32)), (T, E, A, normalize, "agents")
            if normalize:                                   # the statistics in the kernel's own merge order: to the bit
                assert np.array_equal(r["stats"].view(np.int64), st.view(np.int64)), (T, E, A, "agents", r["stats"], st)
